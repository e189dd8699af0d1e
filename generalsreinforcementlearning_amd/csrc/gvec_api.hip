// gvec_api.hip — the C ABI of include/generals_vec.h over the HIP kernels: handle lifetime, streams, size queries and raw
// buffer access, and the helpers of gvec_handle.hpp that every host unit calls.  The entry points of each subsystem are in
// gvec_api_<subsystem>.hip (DESIGN.md "Translation units").  Plain HIP runtime only (no torch, no CPU fallback): every
// compute entry point launches gfx950 kernels and fails with GVEC_E_NO_DEVICE when there is no GPU.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <new>

#include "gvec_handle.hpp"

static thread_local char g_err[512] = "";
void set_err(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}

int32_t DevBuf::in_stage() const {
  if (slot >= 0) return GVEC_OK;
  set_err("a call staged more than %d arguments through its handle", Stage::kSlots);
  return GVEC_E_INVALID;
}

hipError_t DevBuf::alloc(size_t bytes) {
  if (bytes < 16) bytes = 16;
  if (h->stage_cap[slot] < bytes) {
    if (h->stage_ptr[slot]) {
      hipError_t e = hipStreamSynchronize(h->stream);  // an earlier call's copy may still read it
      if (e != hipSuccess) return e;
      (void)hipFree(h->stage_ptr[slot]);
      h->stage_ptr[slot] = nullptr;
      h->stage_cap[slot] = 0;
    }
    const size_t cap = bytes + bytes / 4;  // a little headroom: fewer re-allocations while a caller grows
    hipError_t e = hipMalloc(&h->stage_ptr[slot], cap);
    if (e != hipSuccess) return e;
    h->stage_cap[slot] = cap;
  }
  p = h->stage_ptr[slot];
  return hipSuccess;
}

StepArgs base_args(const gvec_handle* h) {
  StepArgs a = state_args<StepArgs>(h);
  a.legal = h->d_legal;
  a.zeros = h->d_zeros;
  a.pool_hdr = h->p_hdr;
  a.pool_rows = h->p_rows;
  a.pool_army16 = h->p_army16;
  a.pool_army32 = h->p_army32;
  a.num_envs = h->cfg.num_envs;
  a.fd = h->fd;
  a.row_dw = h->row_dw;
  a.mask_dw = h->mask_dw;
  a.pool_size = h->pool_size;
  a.pstride = h->maxp;
  a.prod_general = h->cfg.prod_general;
  a.prod_city = h->cfg.prod_city;
  a.prod_normal = h->cfg.prod_normal;
  a.interval = h->cfg.normal_growth_interval;
  a.interval_magic = (uint32_t)((0x100000000ull + (uint64_t)a.interval - 1) / (uint64_t)a.interval);
  a.turns = 1;
  a.agent_noop = h->agent_noop;
  a.agent_half = h->agent_half;
  a.pool_seed_lo = (uint32_t)h->pool_seed;
  a.pool_seed_hi = (uint32_t)(h->pool_seed >> 32);
  a.env_base = h->env_base;
  if (h->cfg.auto_reset && h->pool_size > 0) a.flags |= KF_AUTORESET;
  // update_stats sums narrow envs' armies with 24-bit multiplies: a turn can merge MAXP armies of 65,535 on one tile
  // before production adds a rate to it, so a rate above 2^24 - 1 - 8 * 65,535 takes the 32-bit sums and no ordinary path
  if (std::max(a.prod_general, std::max(a.prod_city, a.prod_normal)) > 0xFFFFFF - 8 * 65535) a.flags |= KF_BIGRATE;
  return a;
}

int32_t check_status(gvec_handle* h, const char* what) {
  int32_t st = 0;
  HIPCHK(hipMemcpyAsync(&st, h->d_status, sizeof st, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (st != 0) {
    int32_t zero = 0;
    HIPCHK(hipMemcpyAsync(h->d_status, &zero, sizeof zero, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    set_err("%s: input rejected on the device (code %d; -5: board contract - sizes within max_*, owner in [-1, players); "
            "-4: env id out of range)", what, st);
    return st;
  }
  return GVEC_OK;
}

int32_t refresh_legal(gvec_handle* h) {
  StepArgs a = base_args(h);
  HIPCHK(launch_legal(h->var, a, h->stream));
  h->legal_valid = true;
  return GVEC_OK;
}

int32_t import_planes(gvec_handle* h, uint32_t* hdr, uint32_t* rows, uint32_t* army16, int32_t* army32, const int32_t* env_ids_dev, int dst_begin,
                      int n, int dst_envs, const gvec_state_view* v /*device pointers*/, bool fresh, bool init) {
  ImportArgs a;
  memset(&a, 0, sizeof a);
  a.hdr = hdr;
  a.rows = rows;
  a.army16 = army16;
  a.army32 = army32;
  a.zeros = h->d_zeros;
  a.env_ids = env_ids_dev;
  a.dst_begin = dst_begin;
  a.n = n;
  a.dst_envs = dst_envs;
#define GVEC_SRC(field, out, per) a.s_##field = v->field;
  GVEC_VIEW_IMPORTED(GVEC_SRC)
#undef GVEC_SRC
  a.stride = h->stride;
  a.max_p = h->maxp;
  a.max_w = h->cfg.max_width;
  a.max_h = h->cfg.max_height;
  a.fd = h->fd;
  a.row_dw = h->row_dw;
  a.fresh = fresh ? 1u : 0u;
  a.init = init ? 1u : 0u;
  a.fog = h->cfg.fog_of_war ? 1u : 0u;
  a.status = h->d_status;
  HIPCHK(launch_import(h->var, a, h->stream));
  if (init) HIPCHK(launch_setup(h->var, a, h->stream));
  return GVEC_OK;
}

int32_t ensure_device() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    set_err("no HIP device available (%s); this library has no CPU fallback", e == hipSuccess ? "0 devices" : hipGetErrorString(e));
    return GVEC_E_NO_DEVICE;
  }
  return GVEC_OK;
}

// device allocations of a new handle; on failure the caller destroys the handle (which frees what exists)
static int32_t allocate_handle(gvec_handle* h, const gvec_config* cfg) {
  const size_t B = (size_t)cfg->num_envs;
  HIPCHK(hipMalloc(&h->d_hdr, B * HDR_DW * 4));
  HIPCHK(hipMalloc(&h->d_rows, B * h->row_dw * 4));
  HIPCHK(hipMalloc(&h->d_army16, B * h->army_dw * 2));
  HIPCHK(hipMalloc(&h->d_army32, B * h->army_dw * 4));
  HIPCHK(hipMalloc(&h->d_legal, B * h->maxp * h->mask_bytes));
  HIPCHK(hipMalloc(&h->d_actions, B * h->maxp * sizeof(gvec_action)));
  HIPCHK(hipMalloc(&h->d_err, B * 4));
  HIPCHK(hipMalloc(&h->d_status, 16));
  HIPCHK(hipMalloc(&h->d_zeros, (size_t)(h->row_dw + 64) * 4));
  HIPCHK(hipMemset(h->d_zeros, 0, (size_t)(h->row_dw + 64) * 4));
  HIPCHK(hipMalloc(&h->d_counters, 6 * sizeof(unsigned long long)));
  HIPCHK(hipMemset(h->d_rows, 0, B * h->row_dw * 4));
  HIPCHK(hipMemset(h->d_army16, 0, B * h->army_dw * 2));
  HIPCHK(hipMemset(h->d_army32, 0, B * h->army_dw * 4));
  HIPCHK(hipMemset(h->d_legal, 0, B * h->maxp * h->mask_bytes));
  HIPCHK(hipMemset(h->d_actions, 0, B * h->maxp * sizeof(gvec_action)));
  HIPCHK(hipMemset(h->d_err, 0, B * 4));
  HIPCHK(hipMemset(h->d_status, 0, 16));
  {  // every slot starts as a finished 1x1 one-player game, so any kernel is safe before gvec_reset
    std::vector<uint32_t> hdr(B * HDR_DW, 0u);
    for (size_t e = 0; e < B; ++e) {
      uint32_t* x = &hdr[e * HDR_DW];
      x[H_DIMS] = 1u | (1u << 8) | (1u << 16) | ((HF_DONE | (cfg->fog_of_war ? HF_FOG : 0u)) << 24);
      x[H_RECIPW] = 65536u;
      for (int p = 0; p < 8; ++p) x[H_GIDX + p] = 0xFFFFFFFFu;
    }
    HIPCHK(hipMemcpy(h->d_hdr, hdr.data(), hdr.size() * 4, hipMemcpyHostToDevice));
  }
  return GVEC_OK;
}

static size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

// the sizes a handle derives from its config (shared by plain and sharded handles)
static bool set_geometry(gvec_handle* h, const gvec_config* cfg) {
  h->cfg = *cfg;
  h->stride = cfg->max_width * cfg->max_height;
  h->maxp = cfg->max_players;
  if (!pick_variant(cfg->max_players, h->stride, &h->var)) {
    set_err("no kernel variant for %d players / %d tiles", cfg->max_players, h->stride);
    return false;
  }
  // dwords per flat bit-plane: 2*nslot-1 or 2*nslot, so that the step kernel can be compiled for it
  h->fd = (h->stride <= 32 * (2 * h->var.nslot - 1)) ? 2 * h->var.nslot - 1 : 2 * h->var.nslot;
  h->row_dw = (int)round_up((size_t)(3 * h->var.maxp + 13) * h->fd, 4);  // Planes<MAXP>::COUNT planes of fd dwords
  h->army_dw = h->var.nslot * 64;
  h->mask_bytes = 16 * h->fd;  // four direction bit-planes of fd dwords per player
  h->mask_dw = h->mask_bytes / 4;
  h->stream = nullptr;
  return true;
}

extern "C" {

int32_t gvec_abi_version(void) { return GVEC_ABI_VERSION; }
const char* gvec_last_error(void) { return g_err; }

int32_t gvec_config_default(gvec_config* cfg) {
  if (!cfg) return GVEC_E_INVALID;
  memset(cfg, 0, sizeof *cfg);
  cfg->abi_version = GVEC_ABI_VERSION;
  cfg->num_envs = 1;
  cfg->max_width = 20;
  cfg->max_height = 20;
  cfg->max_players = 2;
  cfg->device = 0;
  cfg->fog_of_war = 1;              // engine_initializer.go:118
  cfg->prod_general = 1;            // config.go:206
  cfg->prod_city = 1;               // config.go:207
  cfg->prod_normal = 1;             // config.go:208
  cfg->normal_growth_interval = 25; // config.go:209
  cfg->auto_reset = 0;
  return GVEC_OK;
}

int32_t gvec_create_sharded(const gvec_config* cfg, const int32_t* devices, int32_t num_devices, gvec_handle** out) {
  if (!cfg || !out || !devices || num_devices < 1 || num_devices > 64) return GVEC_E_INVALID;
  *out = nullptr;
  if (cfg->num_envs < num_devices) {
    set_err("gvec_create_sharded: %d envs over %d shards", cfg->num_envs, num_devices);
    return GVEC_E_INVALID;
  }
  RET_IF(ensure_device());
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  for (int i = 0; i < num_devices; ++i)
    if (devices[i] < 0 || devices[i] >= ndev) {
      set_err("gvec_create_sharded: device %d of %d", devices[i], ndev);
      return GVEC_E_INVALID;
    }
  gvec_handle* h = new (std::nothrow) gvec_handle();
  if (!h) return GVEC_E_INVALID;
  gvec_config top = *cfg;
  top.device = devices[0];
  if (cfg->abi_version != GVEC_ABI_VERSION || !set_geometry(h, &top)) {
    delete h;
    return GVEC_E_INVALID;
  }
  h->legal_valid = true;
  const int base = cfg->num_envs / num_devices, rem = cfg->num_envs % num_devices;   // sharding.shard_range
  for (int i = 0; i < num_devices; ++i) {
    auto w = std::make_unique<gvec_handle::ShardWorker>();
    w->n = base + (i < rem ? 1 : 0);
    w->begin = i * base + (i < rem ? i : rem);
    gvec_handle::ShardWorker* wp = w.get();
    w->th = std::thread([wp] { wp->run(); });
    h->shards.push_back(std::move(w));
  }
  for (int i = 0; i < num_devices; ++i) {
    gvec_handle::ShardWorker* wp = h->shards[i].get();
    gvec_config c = *cfg;
    c.num_envs = wp->n;
    c.device = devices[i];
    wp->post([wp, c, devices, num_devices, i]() -> int32_t {
      const int32_t rc = gvec_create(&c, &wp->h);
      if (rc != GVEC_OK) return rc;
      wp->h->env_base = wp->begin;
      for (int j = 0; j < num_devices; ++j)   // direct xGMI copies for the record gather (best effort: already on / same device fail harmlessly)
        if (devices[j] != devices[i]) {
          int can = 0;
          if (hipDeviceCanAccessPeer(&can, devices[i], devices[j]) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(devices[j], 0);
          (void)hipGetLastError();
        }
      return GVEC_OK;
    });
  }
  int32_t rc = GVEC_OK;
  for (auto& w : h->shards) {
    const int32_t r = w->wait();
    if (r < 0 && rc >= 0) {
      rc = r;
      set_err("shard of envs [%d, %d): %s", w->begin, w->begin + w->n, w->err.c_str());
    }
  }
  if (rc != GVEC_OK) {
    std::string keep = g_err;
    (void)gvec_destroy(h);
    set_err("%s", keep.c_str());
    return rc;
  }
  *out = h;
  return GVEC_OK;
}

int32_t gvec_num_shards(const gvec_handle* h) { return h ? (int32_t)h->shards.size() : GVEC_E_INVALID; }

int32_t gvec_shard(gvec_handle* h, int32_t i, gvec_handle** child, int32_t* env_begin, int32_t* n, int32_t* device) {
  if (!h || !h->sharded() || i < 0 || i >= (int32_t)h->shards.size()) return GVEC_E_INVALID;
  const auto& w = h->shards[i];
  if (child) *child = w->h;
  if (env_begin) *env_begin = w->begin;
  if (n) *n = w->n;
  if (device) *device = w->h->cfg.device;
  return GVEC_OK;
}

int32_t gvec_create(const gvec_config* cfg, gvec_handle** out) {
  if (!cfg || !out) return GVEC_E_INVALID;
  *out = nullptr;
  if (cfg->abi_version != GVEC_ABI_VERSION) {
    set_err("abi_version %d != %d", cfg->abi_version, GVEC_ABI_VERSION);
    return GVEC_E_INVALID;
  }
  if (cfg->num_envs < 1 || cfg->max_width < 1 || cfg->max_width > GVEC_MAX_DIM || cfg->max_height < 1 ||
      cfg->max_height > GVEC_MAX_DIM || cfg->max_players < 1 || cfg->max_players > GVEC_MAX_PLAYERS ||
      cfg->normal_growth_interval < 1 || cfg->prod_general < 0 || cfg->prod_city < 0 || cfg->prod_normal < 0 ||
      cfg->prod_general > 0xFFFFFF || cfg->prod_city > 0xFFFFFF || cfg->prod_normal > 0xFFFFFF) {
    set_err("gvec_create: config out of range");
    return GVEC_E_INVALID;
  }
  RET_IF(ensure_device());
  HIPCHK(hipSetDevice(cfg->device));
  gvec_handle* h = new (std::nothrow) gvec_handle();
  if (!h) return GVEC_E_INVALID;
  if (!set_geometry(h, cfg)) {
    delete h;
    return GVEC_E_INVALID;
  }
  {
    const int32_t rc = allocate_handle(h, cfg);
    if (rc != GVEC_OK) {
      (void)gvec_destroy(h);
      return rc;
    }
  }
  h->legal_valid = true;
  *out = h;
  return GVEC_OK;
}

int32_t gvec_destroy(gvec_handle* h) {
  if (!h) return GVEC_E_INVALID;
  if (h->sharded()) {
    for (auto& w : h->shards) {   // each child on the thread that has been driving its device
      gvec_handle::ShardWorker* wp = w.get();
      wp->post([wp]() -> int32_t {
        const int32_t r = wp->h ? gvec_destroy(wp->h) : GVEC_OK;
        wp->h = nullptr;
        return r;
      });
    }
    for (auto& w : h->shards) (void)w->wait();
    for (auto& w : h->shards) w->stop();
    delete h;
    return GVEC_OK;
  }
  (void)hipStreamSynchronize(h->stream);
  void* ptrs[] = {h->d_hdr, h->d_rows, h->d_army16, h->d_army32, h->d_legal, h->d_actions, h->d_err, h->d_status, h->d_zeros, h->d_counters,
                  h->d_snap, h->d_gym_prev, h->p_hdr, h->p_rows, h->p_army16, h->p_army32};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  for (void* p : h->stage_ptr)
    if (p) (void)hipFree(p);
  delete h;
  return GVEC_OK;
}

int32_t gvec_set_stream(gvec_handle* h, void* hip_stream) {
  if (!h) return GVEC_E_INVALID;
  if (h->sharded()) return sharded::unsupported("gvec_set_stream");
  h->stream = reinterpret_cast<hipStream_t>(hip_stream);
  return GVEC_OK;
}
int32_t gvec_synchronize(gvec_handle* h) {
  if (!h) return GVEC_E_INVALID;
  if (h->sharded()) return sharded::fan(h, [](gvec_handle* c, int, int) { return gvec_synchronize(c); });
  HIPCHK(hipStreamSynchronize(h->stream));
  return GVEC_OK;
}

int32_t gvec_host_alloc(uint64_t bytes, void** out) {
  if (!out || bytes == 0) return GVEC_E_INVALID;
  *out = nullptr;
  RET_IF(ensure_device());
  HIPCHK(hipHostMalloc(out, (size_t)bytes, hipHostMallocDefault));
  return GVEC_OK;
}
int32_t gvec_host_free(void* p) {
  if (!p) return GVEC_OK;
  HIPCHK(hipHostFree(p));
  return GVEC_OK;
}

int32_t gvec_num_envs(const gvec_handle* h) { return h ? h->cfg.num_envs : GVEC_E_INVALID; }
int32_t gvec_tile_stride(const gvec_handle* h) { return h ? h->stride : GVEC_E_INVALID; }
int32_t gvec_mask_bytes(const gvec_handle* h) { return h ? h->mask_bytes : GVEC_E_INVALID; }
int64_t gvec_state_bytes_per_env(const gvec_handle* h) {
  return h ? (int64_t)4 * (HDR_DW + h->row_dw + h->army_dw) : (int64_t)GVEC_E_INVALID;
}

int32_t gvec_read_buffer(gvec_handle* h, int32_t which, uint64_t byte_offset, uint64_t bytes, void* host_dst) {
  if (!h || !host_dst) return GVEC_E_INVALID;
  if (h->sharded()) return sharded::unsupported("gvec_read_buffer");
  const size_t B = (size_t)h->cfg.num_envs;
  size_t total = 0;
  const void* base = nullptr;
  switch (which) {
    case GVEC_BUF_HEADER: base = h->d_hdr; total = B * HDR_DW * 4; break;
    case GVEC_BUF_LEGAL: base = h->d_legal; total = B * h->maxp * h->mask_bytes; break;
    case GVEC_BUF_ACTIONS: base = h->d_actions; total = B * h->maxp * sizeof(gvec_action); break;
    case GVEC_BUF_ERR: base = h->d_err; total = B * 4; break;
    default:
      set_err("gvec_read_buffer: buffer %d is not one of header / legal masks / actions / err", which);
      return GVEC_E_INVALID;
  }
  if (byte_offset > total || bytes > total - byte_offset) return GVEC_E_RANGE;
  if (bytes == 0) return GVEC_OK;
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipMemcpyAsync(host_dst, reinterpret_cast<const char*>(base) + byte_offset, (size_t)bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return GVEC_OK;
}

void* gvec_device_buffer(gvec_handle* h, int32_t which) {
  if (!h) return nullptr;
  if (h->sharded()) return nullptr;   // device memory belongs to one device: gvec_device_buffer(gvec_shard(h, i), which)
  switch (which) {
    case 0: return h->d_hdr;
    case 1: return h->d_rows;
    case 2: return h->d_army16;
    case 6: return h->d_army32;
    case 3: return h->d_legal;
    case 4: return h->d_actions;
    case 5: return h->d_err;
    default: return nullptr;
  }
}

int32_t gvec_selftest(int32_t device) {
  RET_IF(ensure_device());
  HIPCHK(hipSetDevice(device));
  int32_t* d = nullptr;
  HIPCHK(hipMalloc(&d, 16));
  HIPCHK(hipMemset(d, 0xFF, 16));
  hipError_t e = launch_selftest(d, nullptr);
  int32_t out = -1;
  if (e == hipSuccess) e = hipMemcpy(&out, d, 4, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) {
    set_err("selftest: %s", hipGetErrorString(e));
    return GVEC_E_HIP;
  }
  if (out != 0) set_err("wave-primitive self-test failed: lane %d check %d", out / 16, out % 16);
  return out;
}

}  // extern "C"
