// gvec_api_state.hip — state in and out of a handle: gvec_state_view reads and writes, player visibility, record slabs and
// env-to-env copies.  Host only (gvec_handle.hpp); the kernels are in gvec_state.hip.
#include "gvec_handle.hpp"

static int32_t export_range(gvec_handle* h, int32_t env_begin, int32_t n, const gvec_state_view* view, int32_t vis_player,
                            uint8_t* pv_visible, uint8_t* pv_fog, int32_t mem) {
  if (!in_range(h, env_begin, n)) return GVEC_E_RANGE;
  if (n == 0) return GVEC_OK;
  HIPCHK(hipSetDevice(h->cfg.device));
  const ViewCounts c = view_counts(h, (size_t)n);
  static const gvec_state_view kEmpty = {};
  const gvec_state_view* v = view ? view : &kEmpty;
  Stage st(h);
  ExportArgs a = state_args<ExportArgs>(h);
  a.env_begin = env_begin;
  a.n = n;
  a.stride = h->stride;
  a.max_p = h->maxp;
  a.fd = h->fd;
  a.row_dw = h->row_dw;
  a.vis_player = vis_player;
#define GVEC_STAGE(field, out, per) RET_IF(stage_out(st.next(), v->field, c.per, mem, &a.out));
  GVEC_VIEW_FIELDS(GVEC_STAGE)
#undef GVEC_STAGE
  DevBuf &b_visible = st.next(), &b_fog = st.next();
  RET_IF(stage_out(b_visible, pv_visible, c.TILE, mem, &a.pv_visible));
  RET_IF(stage_out(b_fog, pv_fog, c.TILE, mem, &a.pv_fog));
  HIPCHK(launch_export(h->var, a, h->stream));
  int i = 0;   // the fields' buffers, in the order they were handed out
#define GVEC_COPY(field, out, per) RET_IF(copy_out(h, st[i++], v->field, c.per, mem));
  GVEC_VIEW_FIELDS(GVEC_COPY)
#undef GVEC_COPY
  RET_IF(copy_out(h, b_visible, pv_visible, c.TILE, mem));
  RET_IF(copy_out(h, b_fog, pv_fog, c.TILE, mem));
  if (mem == GVEC_MEM_HOST) HIPCHK(hipStreamSynchronize(h->stream));
  return GVEC_OK;
}

static RecordArgs record_args(gvec_handle* h, int32_t env_begin, int32_t n, void* slab) {
  RecordArgs a = state_args<RecordArgs>(h);
  char* d = reinterpret_cast<char*>(slab);
  const size_t hb = (size_t)n * HDR_DW * 4, rb = (size_t)n * h->row_dw * 4;
  a.rec_hdr = reinterpret_cast<uint32_t*>(d);
  a.rec_rows = reinterpret_cast<uint32_t*>(d + hb);
  a.rec_army = reinterpret_cast<int32_t*>(d + hb + rb);
  a.env_begin = env_begin;
  a.n = n;
  a.fd = h->fd;
  a.row_dw = h->row_dw;
  a.max_w = h->cfg.max_width;
  a.max_h = h->cfg.max_height;
  a.max_p = h->maxp;
  a.status = h->d_status;
  return a;
}

extern "C" {

int32_t gvec_player_visibility(gvec_handle* h, int32_t player, uint8_t* visible, uint8_t* fog, int32_t mem) {
  if (!h) return GVEC_E_INVALID;
  if (h->sharded()) {
    const size_t st = (size_t)h->stride;
    return sharded::fan_host(h, mem, "gvec_player_visibility", [=](gvec_handle* c, int begin, int) {
      return gvec_player_visibility(c, player, visible ? visible + begin * st : nullptr, fog ? fog + begin * st : nullptr, GVEC_MEM_HOST);
    });
  }
  return export_range(h, 0, h->cfg.num_envs, nullptr, player, visible, fog, mem);
}

int32_t gvec_read_state(gvec_handle* h, int32_t env_begin, int32_t n, const gvec_state_view* view, int32_t mem) {
  if (!h || !view) return GVEC_E_INVALID;
  if (h->sharded()) {
    RET_IF(sharded::host_only(mem, "gvec_read_state"));
    const gvec_state_view v = *view;
    return sharded::fan_range(h, env_begin, n, [=](gvec_handle* c, int lb, int cnt, size_t skip) {
      const gvec_state_view o = sharded::offset_view(c, v, skip);
      return gvec_read_state(c, lb, cnt, &o, GVEC_MEM_HOST);
    });
  }
  return export_range(h, env_begin, n, view, -1, nullptr, nullptr, mem);
}

int32_t gvec_write_state(gvec_handle* h, int32_t env_begin, int32_t n, const gvec_state_view* view, int32_t mem) {
  if (!h || !view) return GVEC_E_INVALID;
  if (h->sharded()) {
    RET_IF(sharded::host_only(mem, "gvec_write_state"));
    const gvec_state_view v = *view;
    return sharded::fan_range(h, env_begin, n, [=](gvec_handle* c, int lb, int cnt, size_t skip) {
      const gvec_state_view o = sharded::offset_view(c, v, skip);
      return gvec_write_state(c, lb, cnt, &o, GVEC_MEM_HOST);
    });
  }
  if (!in_range(h, env_begin, n)) return GVEC_E_RANGE;
  if (n == 0) return GVEC_OK;
  if (view->width || view->height || view->players) {
    set_err("gvec_write_state cannot change board dimensions or player count; use gvec_reset");
    return GVEC_E_INVALID;
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  const ViewCounts c = view_counts(h, (size_t)n);
  Stage st(h);
  gvec_state_view v;
  memset(&v, 0, sizeof v);
  // width, height and players are NULL here and stay so; winner and tile_count are derived, not written
#define GVEC_STAGE(field, out, per) RET_IF(stage_in(h, st.next(), view->field, c.per, mem, &v.field));
  GVEC_VIEW_IMPORTED(GVEC_STAGE)
#undef GVEC_STAGE
  RET_IF(import_planes(h, h->d_hdr, h->d_rows, h->d_army16, h->d_army32, nullptr, env_begin, n, h->cfg.num_envs, &v, false, false));
  RET_IF(check_status(h, "gvec_write_state"));
  return refresh_legal(h);
}

int32_t gvec_export_records(gvec_handle* h, int32_t env_begin, int32_t n, void* dst_device) {
  if (!h || !dst_device) return GVEC_E_INVALID;
  if (h->sharded()) return sharded::unsupported("gvec_export_records");
  if (!in_range(h, env_begin, n)) return GVEC_E_RANGE;
  if (n == 0) return GVEC_OK;
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(launch_records(h->var, record_args(h, env_begin, n, dst_device), false, h->stream));
  return GVEC_OK;
}

int32_t gvec_import_records(gvec_handle* h, int32_t env_begin, int32_t n, const void* src_device) {
  if (!h || !src_device) return GVEC_E_INVALID;
  if (h->sharded()) return sharded::unsupported("gvec_import_records");
  if (!in_range(h, env_begin, n)) return GVEC_E_RANGE;
  if (n == 0) return GVEC_OK;
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(launch_records(h->var, record_args(h, env_begin, n, const_cast<void*>(src_device)), true, h->stream));
  h->legal_valid = false;
  // every record's header was checked on the device before anything was taken from it
  return check_status(h, "gvec_import_records");
}

int32_t gvec_copy_envs(gvec_handle* dst, const int32_t* dst_ids, gvec_handle* src, const int32_t* src_ids, int32_t n) {
  if (!dst) return GVEC_E_INVALID;
  if (!src) src = dst;
  if (n < 0) {
    set_err("gvec_copy_envs: n = %d", n);
    return GVEC_E_INVALID;
  }
  if (dst->sharded() || src->sharded()) return sharded::unsupported("gvec_copy_envs");
  if (n == 0) return GVEC_OK;
  // the same variant, plane stride and army block on both sides, and the same rules for the state to play under
  const gvec_config &dc = dst->cfg, &sc = src->cfg;
  const char* field = dc.device != sc.device ? "device"
                      : dc.max_width != sc.max_width ? "max_width"
                      : dc.max_height != sc.max_height ? "max_height"
                      : dc.max_players != sc.max_players ? "max_players"
                      : dc.prod_general != sc.prod_general ? "prod_general"
                      : dc.prod_city != sc.prod_city ? "prod_city"
                      : dc.prod_normal != sc.prod_normal ? "prod_normal"
                      : dc.normal_growth_interval != sc.normal_growth_interval ? "normal_growth_interval"
                      : nullptr;
  if (field) {
    set_err("gvec_copy_envs: the handles differ in %s", field);
    return GVEC_E_INVALID;
  }
  HIPCHK(hipSetDevice(dc.device));
  if (src->d_gym_prev) RET_IF(ensure_gym_prev(dst));
  if (src->d_snap && !dst->d_snap) RET_IF(ensure_snapshots(dst));
  int snap_dw = 0, record_dw = 0;
  experience_layout(dst->var, dst->fd, &snap_dw, &record_dw);
  CopyArgs a;
  memset(&a, 0, sizeof a);
  a.d_hdr = dst->d_hdr;
  a.d_rows = dst->d_rows;
  a.d_army16 = dst->d_army16;
  a.d_army32 = dst->d_army32;
  a.d_prev = dst->d_gym_prev;
  a.d_snap = dst->d_snap;
  a.s_hdr = src->d_hdr;
  a.s_rows = src->d_rows;
  a.s_army16 = src->d_army16;
  a.s_army32 = src->d_army32;
  a.s_prev = src->d_gym_prev;
  a.s_snap = src->d_snap;
  a.dst_ids = dst_ids;
  a.src_ids = src_ids;
  a.n = n;
  a.dst_envs = dc.num_envs;
  a.src_envs = sc.num_envs;
  a.row_dw = dst->row_dw;
  a.army_dw = dst->army_dw;
  a.prev_dw = 3 * dst->var.maxp;
  a.snap_dw = snap_dw;
  a.status = dst->d_status;
  // ordered after the work already enqueued on src's stream; src's next call waits for the copy in turn
  const bool cross = src != dst && src->stream != dst->stream;
  hipEvent_t ev = nullptr;
  if (cross) {
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, src->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(dst->stream, ev, 0);
    if (e != hipSuccess) {
      (void)hipEventDestroy(ev);
      HIPCHK(e);
    }
  }
  hipError_t e = launch_copy_envs(a, dst->stream);
  if (cross) {
    if (e == hipSuccess) e = hipEventRecord(ev, dst->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(src->stream, ev, 0);
    (void)hipEventDestroy(ev);  // released once the recorded work completes
  }
  HIPCHK(e);
  // the per-turn agent samples from d_legal: the copied rows of it are stale
  dst->legal_valid = false;
  return check_status(dst, "gvec_copy_envs");
}

}  // extern "C"
