// gvec_handle.hpp — what the host units of the C ABI (gvec_api*.hip, DESIGN.md "Translation units") share: the handle,
// error reporting, argument checks, host staging, the gvec_state_view field table and the sharded fan-out.
// Host only: no kernel unit includes it, and no unit that includes it defines a kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gvec_launch.hpp"

using namespace gvec;

// internal to libgvec_hip.so: the library exports the C ABI of include/generals_vec.h and nothing of this header
#pragma GCC visibility push(hidden)

// gvec_last_error()'s message: one thread_local buffer, defined (with set_err) in gvec_api.hip
void set_err(const char* fmt, ...);

#define HIPCHK(expr)                                                                   \
  do {                                                                                 \
    hipError_t e__ = (expr);                                                           \
    if (e__ != hipSuccess) {                                                           \
      set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
      (void)hipGetLastError(); /* reported: do not leave it for the next launch's error check */ \
      return GVEC_E_HIP;                                                               \
    }                                                                                  \
  } while (0)

#define RET_IF(x)                \
  do {                           \
    int32_t r__ = (x);           \
    if (r__ != GVEC_OK) return r__; \
  } while (0)

struct gvec_handle {
  gvec_config cfg;
  Variant var;
  int stride, fd, row_dw, mask_dw, mask_bytes, army_dw, maxp;
  hipStream_t stream;
  uint32_t* d_hdr = nullptr;
  uint32_t* d_rows = nullptr;
  uint32_t* d_army16 = nullptr;  // narrow armies (u16 pairs), army_dw / 2 dwords per env
  int32_t* d_army32 = nullptr;   // wide escape (int32), army_dw dwords per env: only envs flagged HF_WIDE use it
  uint32_t* d_legal = nullptr;
  gvec_action* d_actions = nullptr;
  int32_t* d_err = nullptr;
  int32_t* d_status = nullptr;
  uint32_t* d_zeros = nullptr;  // row_dw zero dwords (StepArgs::zeros)
  uint32_t agent_noop = 6554u, agent_half = 19661u;  // gvec_set_agent_mix
  unsigned long long* d_counters = nullptr;  // [6]: before[3], after[3]
  uint32_t* d_snap = nullptr;                // experience snapshots [B][snap_dw] (allocated on first use)
  int snap_dw = 0, record_dw = 0;
  bool record_actions = false;               // per-turn rollouts write the agent's moves into d_actions
  int32_t* d_gym_prev = nullptr;             // [B][3*MAXP] player stats as of the previous gvec_gym_observe
  uint32_t* p_hdr = nullptr;
  uint32_t* p_rows = nullptr;
  uint32_t* p_army16 = nullptr;
  int32_t* p_army32 = nullptr;
  int pool_size = 0;
  uint64_t pool_seed = 0;
  bool legal_valid = false;
  // grow-only device staging for GVEC_MEM_HOST calls, handed out to a call's staged arguments by its Stage.
  // Owned by the handle, reused by every call (work on one handle is serialised on its stream), freed by
  // gvec_destroy - the host path allocates nothing in steady state.
  static constexpr int kStageSlots = 24;
  void* stage_ptr[kStageSlots] = {};
  size_t stage_cap[kStageSlots] = {};
  // ---- sharding (gvec_create_sharded) ----
  int env_base = 0;                 // a shard's first env within the sharded batch: keys its agent / pool / map draws
  struct ShardWorker;
  std::vector<std::unique_ptr<ShardWorker>> shards;   // non-empty: this handle owns no device memory, only its shards
  bool sharded() const { return !shards.empty(); }
};

// One worker thread per shard: every call on a sharded handle posts one task per shard and waits for all of them, so the
// shards' host copies, launches and synchronisations run concurrently (a GVEC_MEM_HOST call on a single-device handle ends
// in a stream synchronise; calling the shards one after the other would serialise the devices).  A child handle is only
// ever touched by its own worker: the "not thread-safe per handle" rule holds for every one of them.
struct gvec_handle::ShardWorker {
  gvec_handle* h = nullptr;   // a plain single-device handle
  int begin = 0, n = 0;       // envs [begin, begin + n) of the sharded batch
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::function<int32_t()> task;
  bool has_task = false, done = false, quit = false;
  int32_t rc = 0;
  std::string err;

  void run() {
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] { return has_task || quit; });
      if (quit) return;
      std::function<int32_t()> f = std::move(task);
      has_task = false;
      lk.unlock();
      const int32_t r = f();
      const char* e = gvec_last_error();   // this thread's own message
      lk.lock();
      rc = r;
      err = (r < 0 && e) ? e : "";
      done = true;
      cv.notify_all();
    }
  }
  void post(std::function<int32_t()> f) {
    std::lock_guard<std::mutex> lk(mu);
    task = std::move(f);
    has_task = true;
    done = false;
    cv.notify_all();
  }
  int32_t wait() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return done; });
    return rc;
  }
  void stop() {
    {
      std::lock_guard<std::mutex> lk(mu);
      quit = true;
      cv.notify_all();
    }
    if (th.joinable()) th.join();
  }
};

// ---- helpers every unit calls; those not defined here live in gvec_api.hip ----
int32_t ensure_device();                              // GVEC_E_NO_DEVICE without a GPU
StepArgs base_args(const gvec_handle* h);
int32_t check_status(gvec_handle* h, const char* what);   // reads (and clears) the device status word; synchronises
int32_t refresh_legal(gvec_handle* h);                // the internal legal-mask buffer from the resident state
int32_t import_planes(gvec_handle* h, uint32_t* hdr, uint32_t* rows, uint32_t* army16, int32_t* army32, const int32_t* env_ids_dev, int dst_begin,
                      int n, int dst_envs, const gvec_state_view* v /*device pointers*/, bool fresh, bool init);
int32_t ensure_snapshots(gvec_handle* h);             // gvec_api_experience.hip: d_snap, on first use
int32_t ensure_gym_prev(gvec_handle* h);              // gvec_api_gym.hip: d_gym_prev, on first use

// zeroed launch arguments of type A over the handle's resident state
template <typename A>
A state_args(const gvec_handle* h) {
  A a{};
  a.hdr = h->d_hdr;
  a.rows = h->d_rows;
  a.army16 = h->d_army16;
  a.army32 = h->d_army32;
  return a;
}

inline bool in_range(const gvec_handle* h, int32_t env_begin, int32_t n) { return env_begin >= 0 && n >= 0 && env_begin + n <= h->cfg.num_envs; }

inline int32_t null_args(const char* fn) {
  set_err("%s: args or a required pointer is NULL", fn);
  return GVEC_E_INVALID;
}

inline int32_t check_scratch(const char* fn, const void* scratch) {
  if (reinterpret_cast<uintptr_t>(scratch) & 15) {
    set_err("%s: scratch must be 16-byte aligned", fn);
    return GVEC_E_INVALID;
  }
  return GVEC_OK;
}

// the agent's draw of one call
inline void set_agent_seed(StepArgs* a, uint64_t seed, int32_t invalid_permille) {
  a->seed_lo = (uint32_t)seed;
  a->seed_hi = (uint32_t)(seed >> 32);
  a->invalid_permille = invalid_permille;
}

// how a handle-free entry point ends, once its arguments have passed: `launch` on `device`.  A macro, so that a failure
// names the launcher (HIPCHK prints its expression)
#define ON_DEVICE(device, launch)   \
  do {                              \
    RET_IF(ensure_device());        \
    HIPCHK(hipSetDevice(device));   \
    HIPCHK(launch);                 \
    return GVEC_OK;                 \
  } while (0)

// ---- gvec_state_view, field by field ----
// X(field, its name in ExportArgs, elements per env), where TILE = max_width * max_height, PLAYER = max_players and ENV = 1.
// IMPORTED are the fields a caller may hand in (ImportArgs::s_<field>); winner and tile_count are derived from them and
// only ever come out.
#define GVEC_VIEW_IMPORTED(X)                                                                                                     \
  X(army, army_out, TILE) X(owner, owner, TILE) X(type, type, TILE) X(visible, visible, TILE) X(listed, listed, TILE)             \
  X(changed, changed, TILE) X(vis_changed, vis_changed, TILE) X(turn, turn, ENV) X(done, done, ENV) X(width, width, ENV)           \
  X(height, height, ENV) X(players, players, ENV) X(alive, alive, PLAYER) X(army_count, army_count, PLAYER)                        \
  X(general_idx, general_idx, PLAYER)
#define GVEC_VIEW_FIELDS(X) GVEC_VIEW_IMPORTED(X) X(winner, winner, ENV) X(tile_count, tile_count, PLAYER)

struct ViewCounts {
  size_t TILE, PLAYER, ENV;
};
// elements of a field of each kind over n envs
inline ViewCounts view_counts(const gvec_handle* h, size_t n) { return {n * (size_t)h->stride, n * (size_t)h->maxp, n}; }

// ---- host staging ----
// One staged argument of the current call: a view of one slot of the handle's grow-only staging.
struct DevBuf {
  gvec_handle* h = nullptr;
  int slot = -1;   // -1: the call asked its Stage for more slots than there are
  void* p = nullptr;
  int32_t in_stage() const;       // GVEC_E_INVALID for the buffer past a Stage's last slot
  hipError_t alloc(size_t bytes);
  template <typename T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

// Hands a call its staging slots in order, so that two buffers alive in one call never share one.  A helper that stages
// inside another call's staging takes the caller's Stage and goes on from where that stands.
class Stage {
 public:
  static constexpr int kSlots = gvec_handle::kStageSlots - 1;
  explicit Stage(gvec_handle* h) : h_(h) {}
  DevBuf& next() {
    if (used_ == kSlots) return none_;   // STAGE_ALLOC on it fails with GVEC_E_INVALID
    bufs_[used_] = DevBuf{h_, used_};
    return bufs_[used_++];
  }
  DevBuf& operator[](int i) { return bufs_[i]; }   // the i-th buffer handed out
  // the one slot no Stage hands out: for a buffer that has to outlive a nested public call, which starts a Stage of its own
  static DevBuf reserved(gvec_handle* h) { return DevBuf{h, kSlots}; }

 private:
  gvec_handle* h_;
  int used_ = 0;
  DevBuf bufs_[kSlots], none_;
};

// grows a staged argument's buffer to `bytes`
#define STAGE_ALLOC(buf, bytes) \
  do {                          \
    RET_IF(buf.in_stage());     \
    HIPCHK(buf.alloc(bytes));   \
  } while (0)

// a caller's input array on the device: itself (device memory) or a staged copy (host memory); null stays null.
// U is T or const T: the pointers of a gvec_state_view are not const
template <typename T, typename U>
int32_t stage_in(gvec_handle* h, DevBuf& buf, const T* src, size_t count, int32_t mem, U** out) {
  *out = nullptr;
  if (!src) return GVEC_OK;
  if (mem == GVEC_MEM_DEVICE) {
    *out = const_cast<U*>(src);
    return GVEC_OK;
  }
  STAGE_ALLOC(buf, count * sizeof(T));
  HIPCHK(hipMemcpyAsync(buf.p, src, count * sizeof(T), hipMemcpyHostToDevice, h->stream));
  *out = buf.as<T>();
  return GVEC_OK;
}

// where a kernel writes a caller's output array: the array itself or a staged buffer that copy_out brings home
template <typename T>
int32_t stage_out(DevBuf& buf, T* dst, size_t count, int32_t mem, T** out) {
  *out = nullptr;
  if (!dst) return GVEC_OK;
  if (mem == GVEC_MEM_DEVICE) {
    *out = dst;
    return GVEC_OK;
  }
  STAGE_ALLOC(buf, count * sizeof(T));
  *out = buf.as<T>();
  return GVEC_OK;
}

template <typename T>
int32_t copy_out(gvec_handle* h, const DevBuf& buf, T* dst, size_t count, int32_t mem) {
  if (!dst || mem == GVEC_MEM_DEVICE) return GVEC_OK;
  HIPCHK(hipMemcpyAsync(dst, buf.p, count * sizeof(T), hipMemcpyDeviceToHost, h->stream));
  return GVEC_OK;
}

// =========================================================================================================================
// Sharded handles (gvec_create_sharded): one handle over several devices, SURVEY 8(b) "one handle may span several GPUs".
// Boards are independent, so shard i simply IS envs [begin_i, begin_i + n_i) of the batch (contiguous, sizes differing by
// at most one: the shard_range rule of sharding.py), resident on its own device for the whole run; no call moves board
// state between devices.  Every GVEC_MEM_HOST entry point fans out to the shards with the caller's arrays offset to the
// shard's range, all shards working at once on their own threads and streams.  Because a shard folds its offset into the
// agent / pool / map keys (env_base), the batch plays the same games whatever the number of shards:
// tests/test_hip_sharded.py holds a 3-shard handle against a single-device one bit for bit.
// Entry points that take DEVICE pointers belong to one device: use them on gvec_shard(h, i).
// =========================================================================================================================
namespace sharded {

template <typename F>  // F(gvec_handle* child, int begin, int n) -> int32_t; copied into every shard's task
int32_t fan(gvec_handle* h, F f) {
  for (auto& w : h->shards) {
    gvec_handle::ShardWorker* wp = w.get();
    wp->post([f, wp]() { return f(wp->h, wp->begin, wp->n); });
  }
  int32_t rc = GVEC_OK;
  for (auto& w : h->shards) {
    const int32_t r = w->wait();
    if (r < 0 && rc >= 0) {
      rc = r;
      set_err("shard of envs [%d, %d) on device %d: %s", w->begin, w->begin + w->n, w->h ? w->h->cfg.device : -1, w->err.c_str());
    }
  }
  return rc;
}

// the ordinal of the shard that starts at env `begin` (a handful of shards: linear search)
inline int ordinal_of(const gvec_handle* h, int begin) {
  for (size_t k = 0; k < h->shards.size(); ++k)
    if (h->shards[k]->begin == begin) return (int)k;
  return 0;
}

inline int32_t host_only(int32_t mem, const char* what) {
  if (mem == GVEC_MEM_HOST) return GVEC_OK;
  set_err("%s with device pointers on a sharded handle: device memory belongs to one device - call it on gvec_shard(h, i)", what);
  return GVEC_E_INVALID;
}
inline int32_t unsupported(const char* what) {
  set_err("%s works on one device: call it on gvec_shard(h, i)", what);
  return GVEC_E_INVALID;
}

// a call whose per-env host arrays every shard takes its own part of: f(child, begin, n) offsets them by `begin` envs
template <typename F>
int32_t fan_host(gvec_handle* h, int32_t mem, const char* what, F f) {
  RET_IF(host_only(mem, what));
  return fan(h, f);
}

// the part of a caller's view that covers `skip` envs further on
inline gvec_state_view offset_view(const gvec_handle* h, gvec_state_view v, size_t skip) {
  const ViewCounts c = view_counts(h, skip);
#define GVEC_OFF(field, out, per) if (v.field) v.field += c.per;
  GVEC_VIEW_FIELDS(GVEC_OFF)
#undef GVEC_OFF
  return v;
}

// envs [env_begin, env_begin + n) of the batch, split over the shards: f(child, local_begin, count, envs before this piece)
template <typename F>
int32_t fan_range(gvec_handle* h, int32_t env_begin, int32_t n, F f) {
  if (!in_range(h, env_begin, n)) return GVEC_E_RANGE;
  return fan(h, [=](gvec_handle* c, int begin, int cn) -> int32_t {
    const int lo = env_begin > begin ? env_begin : begin, hi = (env_begin + n) < (begin + cn) ? (env_begin + n) : (begin + cn);
    if (hi <= lo) return GVEC_OK;
    return f(c, lo - begin, hi - lo, (size_t)(lo - env_begin));
  });
}

}  // namespace sharded

#pragma GCC visibility pop
