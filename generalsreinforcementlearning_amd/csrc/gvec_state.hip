// gvec_state.hip — the resident state's way in and out: import from planes, export to planes, record slabs, env-to-env copies.
#include "gvec_dispatch.hpp"
#include "gvec_turn.hpp"

namespace gvec {

// =========================================================================================
// import: planes -> resident record (gvec_reset / gvec_write_state / pool build)
// =========================================================================================
template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void import_kernel(ImportArgs A) {
  using B = Board<MAXP, NSLOT>;
  const int lane = lane_id();
  const int i = wave_item();
  if (i >= A.n) return;
  const int env = A.env_ids ? uni(A.env_ids[i]) : A.dst_begin + i;
  if (env < 0 || env >= A.dst_envs) {  // ids handed over in device memory were not seen by the host
    if (lane == 0) atomicExch(A.status, GVEC_E_RANGE);
    return;
  }
  uint32_t* hdr = A.hdr + (size_t)env * HDR_DW;
  uint32_t* rows = A.rows + (size_t)env * A.row_dw;
  const ArmyRef army = army_ref<NSLOT>(A.army16, A.army32, env);
  const size_t to = (size_t)i * A.stride, po = (size_t)i * A.max_p;

  B b;
  if (A.fresh) {
    b.W = A.s_width[i];
    b.H = A.s_height[i];
    b.P = A.s_players[i];
    bool bad = b.W < 1 || b.W > A.max_w || b.H < 1 || b.H > A.max_h || b.P < 1 || b.P > A.max_p || b.P > MAXP;
    if (bad) {
      if (lane == 0) atomicExch(A.status, GVEC_E_INVALID);
      return;
    }
    b.N = b.W * b.H;
    b.recipW = (65536 + b.W - 1) / b.W;
    b.turn = 0;
    b.hflags = A.fog ? HF_FOG : 0u;
    b.alive = (1u << b.P) - 1u;  // initializePlayers: Alive = true (engine_initializer.go:125-143)
    b.hv = (lane >= H_GIDX && lane < H_GIDX + 8) ? 0xFFFFFFFFu : 0u;  // GeneralIdx -1, counters / episode 0
#pragma unroll
    for (int p = 0; p < MAXP; ++p) b.own[p] = b.lst[p] = b.vis[p] = 0u;
    b.chg = b.vch = b.gen = b.city = b.mtn = 0u;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) b.army[s] = 0;
  } else {
    load_board(b, hdr, rows, army, A.fd);
  }
  b.geometry();

  // per-tile source planes are read coalesced in the tile domain (lane l, slot s = tile 64s+l);
  // each predicate becomes a flat plane through the wave ballot
  bool bad_owner = false;
  if (A.s_owner) {
#pragma unroll
    for (int p = 0; p < MAXP; ++p) b.own[p] = 0u;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const int t = 64 * s + lane;
      const int o = (t < b.N) ? (int)A.s_owner[to + t] : -1;
      bad_owner |= (o < -1) || (o >= b.P);
#pragma unroll
      for (int p = 0; p < MAXP; ++p) ballot_to_row0(b.own[p], __builtin_amdgcn_ballot_w64(o == p), s);
    }
  }
  if (wave_any(bad_owner)) {
    if (lane == 0) atomicExch(A.status, GVEC_E_BOARD);
    return;
  }
  if (A.s_type) {
    b.gen = b.city = b.mtn = 0u;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const int t = 64 * s + lane;
      const int ty = (t < b.N) ? (int)A.s_type[to + t] : GVEC_TILE_NORMAL;
      ballot_to_row0(b.gen, __builtin_amdgcn_ballot_w64(ty == GVEC_TILE_GENERAL), s);
      ballot_to_row0(b.city, __builtin_amdgcn_ballot_w64(ty == GVEC_TILE_CITY), s);
      ballot_to_row0(b.mtn, __builtin_amdgcn_ballot_w64(ty == GVEC_TILE_MOUNTAIN), s);
    }
  }
  if (A.s_visible) {
#pragma unroll
    for (int p = 0; p < MAXP; ++p) b.vis[p] = 0u;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const int t = 64 * s + lane;
      const uint32_t v = (t < b.N) ? (uint32_t)A.s_visible[to + t] : 0u;
#pragma unroll
      for (int p = 0; p < MAXP; ++p) ballot_to_row0(b.vis[p], __builtin_amdgcn_ballot_w64(((v >> p) & 1u) != 0u), s);
    }
  }
  if (A.s_listed) {
#pragma unroll
    for (int p = 0; p < MAXP; ++p) b.lst[p] = 0u;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const int t = 64 * s + lane;
      const int o = (t < b.N) ? (int)A.s_listed[to + t] : -1;
#pragma unroll
      for (int p = 0; p < MAXP; ++p) ballot_to_row0(b.lst[p], __builtin_amdgcn_ballot_w64(o == p), s);
    }
  }
  if (A.s_changed) {
    b.chg = 0u;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const int t = 64 * s + lane;
      ballot_to_row0(b.chg, __builtin_amdgcn_ballot_w64(t < b.N && A.s_changed[to + t] != 0), s);
    }
  }
  if (A.s_vis_changed) {
    b.vch = 0u;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const int t = 64 * s + lane;
      ballot_to_row0(b.vch, __builtin_amdgcn_ballot_w64(t < b.N && A.s_vis_changed[to + t] != 0), s);
    }
  }
  if (A.s_army) {
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const int t = 64 * s + lane;
      b.army[s] = (t < b.N) ? A.s_army[to + t] : 0;
    }
  }
  if (A.s_turn) b.turn = A.s_turn[i];
  if (A.s_done) b.hflags = A.s_done[i] ? (b.hflags | HF_DONE) : (b.hflags & ~HF_DONE);
  if (A.s_alive) {
    uint32_t al = 0u;
    for (int p = 0; p < b.P; ++p) al |= (A.s_alive[po + p] ? 1u : 0u) << p;
    b.alive = al;
  }
  for (int p = 0; p < b.P; ++p) {
    if (A.s_army_count) hdr_set(b, H_ARMYCNT + p, (uint32_t)A.s_army_count[po + p]);
    if (A.s_general_idx) hdr_set(b, H_GIDX + p, (uint32_t)A.s_general_idx[po + p]);
  }
  // the planes that are functions of the board: rebuilt on every import (the type planes may have changed)
  derive_targets(b);
  b.static_flags();
  b.refresh_gt1();
  if (A.init) b.hflags |= HF_SETUP;  // performInitialSetup runs in setup_kernel, on the turn engine's layout
  store_army(b, army);
  settle_lists(b);
  b.store_hdr(hdr, A.fresh ? 0u : ((hdr_get(b, H_STATUS) >> 16) & 0xFFu));
  b.store_planes(rows, A.fd, A.row_dw, true);
}

// =========================================================================================
// export: resident record -> planes (gvec_read_state / gvec_player_visibility)
// =========================================================================================
template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void export_kernel(ExportArgs A) {
  using B = Board<MAXP, NSLOT>;
  const int lane = lane_id();
  const int i = wave_item();
  if (i >= A.n) return;
  const int env = A.env_begin + i;
  B b;
  load_board(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd);
  const size_t to = (size_t)i * A.stride, po = (size_t)i * A.max_p;
  const uint32_t special = b.gen | b.city | b.mtn;
  uint32_t pv_plane = 0u;
#pragma unroll
  for (int p = 0; p < MAXP; ++p) pv_plane = (p == A.vis_player) ? b.vis[p] : pv_plane;
  const bool fog_on = (b.hflags & HF_FOG) != 0u;
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) {
    const int t = 64 * s + lane;
    const bool in = t < b.N;
    int owner = -1, listed = -1;
    uint32_t visb = 0u;
#pragma unroll
    for (int p = 0; p < MAXP; ++p) {
      owner = gather(b.own[p], s) ? p : owner;
      listed = gather(b.lst[p], s) ? p : listed;
      visb |= gather(b.vis[p], s) << p;
    }
    // every gather is a cross-lane ds_bpermute: evaluate them all convergently, never inside a
    // per-lane short-circuit (a masked-off source lane reads back as 0)
    const uint32_t is_gen = gather(b.gen, s), is_city = gather(b.city, s), is_mtn = gather(b.mtn, s);
    const int type = is_gen ? GVEC_TILE_GENERAL : (is_city ? GVEC_TILE_CITY : (is_mtn ? GVEC_TILE_MOUNTAIN : GVEC_TILE_NORMAL));
    const uint32_t c = gather(b.chg, s), vc = gather(b.vch, s);
    const uint32_t pv = gather(pv_plane, s), sp = gather(special, s);
    if (t < A.stride) {
      if (A.army_out) A.army_out[to + t] = in ? b.army[s] : 0;
      if (A.owner) A.owner[to + t] = (int8_t)(in ? owner : -1);
      if (A.type) A.type[to + t] = (uint8_t)(in ? type : 0);
      if (A.visible) A.visible[to + t] = (uint8_t)(in ? visb : 0u);
      if (A.listed) A.listed[to + t] = (int8_t)(in ? listed : -1);
      if (A.changed) A.changed[to + t] = (uint8_t)(in ? c : 0u);
      if (A.vis_changed) A.vis_changed[to + t] = (uint8_t)(in ? vc : 0u);
      // ComputePlayerVisibilityOptimized (visibility_optimized.go:166-195)
      if (A.pv_visible) A.pv_visible[to + t] = (uint8_t)(in ? (fog_on ? pv : 1u) : 0u);
      if (A.pv_fog) A.pv_fog[to + t] = (uint8_t)((in && fog_on && !pv && sp) ? 1u : 0u);
    }
  }
  uint32_t tcnt[MAXP];
#pragma unroll
  for (int p = 0; p < MAXP; ++p) tcnt[p] = wave_sum((uint32_t)__builtin_popcount(b.lst[p]));
  if (lane == 0) {
    if (A.turn) A.turn[i] = b.turn;
    if (A.done) A.done[i] = (uint8_t)((b.hflags & HF_DONE) ? 1 : 0);
    // Engine.GetWinner re-derives the winner from the CURRENT Alive flags (engine.go:248-263)
    const int na = __builtin_popcount(b.alive);
    if (A.winner) A.winner[i] = (int8_t)(((b.hflags & HF_DONE) && b.P > 1 && na == 1) ? (31 - __builtin_clz(b.alive)) : -1);
    if (A.width) A.width[i] = b.W;
    if (A.height) A.height[i] = b.H;
    if (A.players) A.players[i] = b.P;
  }
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    if (lane == 0 && p < A.max_p) {
      const bool live = p < b.P;
      if (A.alive) A.alive[po + p] = (uint8_t)(live ? ((b.alive >> p) & 1u) : 0u);
      if (A.army_count) A.army_count[po + p] = live ? (int32_t)hdr_get(b, H_ARMYCNT + p) : 0;
      if (A.tile_count) A.tile_count[po + p] = live ? (int32_t)tcnt[p] : 0;
      if (A.general_idx) A.general_idx[po + p] = live ? (int32_t)hdr_get(b, H_GIDX + p) : -1;
    }
  }
}

// =========================================================================================
// resident records <-> canonical record slabs (gvec_export_records / gvec_import_records): a slab is
// [n][HDR_DW] headers | [n][row_dw] planes | [n][NSLOT*64] int32 armies - always the wide form, whatever the
// env's storage.  Import validates the header of every record before anything is trusted (a slab may come
// from another rank or from a file).
// =========================================================================================
template <int MAXP, int NSLOT, bool IMPORT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void records_kernel(RecordArgs A) {
  using B = Board<MAXP, NSLOT>;
  const int lane = lane_id();
  const int i = wave_item();
  if (i >= A.n) return;
  const int env = A.env_begin + i;
  uint32_t* rec_hdr = A.rec_hdr + (size_t)i * HDR_DW;
  uint32_t* rec_rows = A.rec_rows + (size_t)i * A.row_dw;
  int32_t* rec_army = A.rec_army + (size_t)i * NSLOT * 64;
  B b;
  if constexpr (!IMPORT) {
    load_board(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd);
    b.hflags &= ~HF_WIDE;
    army_store_wide<NSLOT>(b.army, rec_army);
    settle_lists(b);
    b.store_hdr(rec_hdr, (hdr_get(b, H_STATUS) >> 16) & 0xFFu);
    b.store_planes(rec_rows, A.fd, A.row_dw, true, true);  // a record carries its list planes whatever the flag says
  } else {
    b.load_hdr(rec_hdr);
    const bool bad = b.W < 1 || b.W > A.max_w || b.H < 1 || b.H > A.max_h || b.P < 1 || b.P > A.max_p || b.P > MAXP ||
                     b.recipW != (65536 + (b.W > 0 ? b.W : 1) - 1) / (b.W > 0 ? b.W : 1) || (b.alive >> b.P) != 0u;
    if (bad) {
      if (lane == 0) atomicExch(A.status, GVEC_E_BOARD);
      return;
    }
    b.hflags &= (HF_DONE | HF_FOG | HF_LDIFF);  // HF_LDIFF: where load_planes takes the lists from
    army_load_wide<NSLOT>(b.army, rec_army);
    b.load_planes(rec_rows, A.fd);
    b.geometry();  // the constant planes are rebuilt, never taken from the slab
    // nothing outside the board may be set: the turn logic relies on it
#pragma unroll
    for (int p = 0; p < MAXP; ++p) {
      const uint32_t keep = (p < b.P) ? b.valid : 0u;
      b.own[p] &= keep;
      b.lst[p] &= keep;
      b.vis[p] &= keep;
    }
    b.chg &= b.valid;
    b.vch &= b.valid;
    b.gen &= b.valid;
    b.city &= b.valid;
    b.mtn &= b.valid;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) b.army[s] = (64 * s + lane < b.N) ? b.army[s] : 0;
    derive_targets(b);
    b.static_flags();
    b.refresh_gt1();
    store_army(b, army_ref<NSLOT>(A.army16, A.army32, env));
    settle_lists(b);
    b.store_hdr(A.hdr + (size_t)env * HDR_DW, (hdr_get(b, H_STATUS) >> 16) & 0xFFu);
    b.store_planes(A.rows + (size_t)env * A.row_dw, A.fd, A.row_dw, true);
  }
}

// =========================================================================================
// gvec_copy_envs: env dst_ids[i] of one handle becomes env src_ids[i] of another (or of the same) handle, one wave per
// pair.  Every block of the resident layout is moved as it is stored, in 16-byte pieces: the 96-byte header (less the
// slot's lifetime counters), the planes block (row_dw is a multiple of 4), the army block in the form the source header
// names (narrow NSLOT*128 bytes or wide NSLOT*256 bytes, the destination's block of the same form), then the small
// per-env rows of the gym reward baseline and the experience snapshot in dwords.  Plain stores: the destination lines
// stay in L2 for the step that usually follows.
// =========================================================================================
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void copy_envs_kernel(CopyArgs A) {
  const int lane = lane_id();
  const int i = wave_item();
  if (i >= A.n) return;
  const int d = uni(A.dst_ids ? A.dst_ids[i] : i), s = uni(A.src_ids ? A.src_ids[i] : i);
  if (d < 0 || d >= A.dst_envs || s < 0 || s >= A.src_envs) {
    if (lane == 0) atomicExch(A.status, GVEC_E_RANGE);
    return;
  }
  // header: six pieces; the last one holds H_RECIPW and the three H_CNT_* words, which stay the destination's
  static_assert(HDR_DW == 24 && H_RECIPW == 20 && H_CNT_STEPS == 21 && H_CNT_DONE == 23, "copy_envs_kernel: header layout");
  const u32x4* sh = reinterpret_cast<const u32x4*>(A.s_hdr + (size_t)s * HDR_DW);
  u32x4* dh = reinterpret_cast<u32x4*>(A.d_hdr + (size_t)d * HDR_DW);
  const bool wide = ((A.s_hdr[(size_t)s * HDR_DW + H_DIMS] >> 24) & HF_WIDE) != 0u;
  if (lane < HDR_DW / 4) {
    u32x4 v = sh[lane];
    if (lane == HDR_DW / 4 - 1) {
      const u32x4 keep = dh[lane];
      v.y = keep.y;
      v.z = keep.z;
      v.w = keep.w;
    }
    dh[lane] = v;
  }
  {
    const u32x4* sr = reinterpret_cast<const u32x4*>(A.s_rows + (size_t)s * A.row_dw);
    u32x4* dr = reinterpret_cast<u32x4*>(A.d_rows + (size_t)d * A.row_dw);
    for (int k = lane; k < A.row_dw / 4; k += 64) dr[k] = sr[k];
  }
  if (wide) {
    const u32x4* sa = reinterpret_cast<const u32x4*>(A.s_army32 + (size_t)s * A.army_dw);
    u32x4* da = reinterpret_cast<u32x4*>(A.d_army32 + (size_t)d * A.army_dw);
    for (int k = lane; k < A.army_dw / 4; k += 64) da[k] = sa[k];
  } else {
    const u32x4* sa = reinterpret_cast<const u32x4*>(A.s_army16 + (size_t)s * (A.army_dw / 2));
    u32x4* da = reinterpret_cast<u32x4*>(A.d_army16 + (size_t)d * (A.army_dw / 2));
    for (int k = lane; k < A.army_dw / 8; k += 64) da[k] = sa[k];
  }
  if (A.d_prev) {  // a source without the row reads as zeros
    int32_t* dp = A.d_prev + (size_t)d * A.prev_dw;
    for (int k = lane; k < A.prev_dw; k += 64) dp[k] = A.s_prev ? A.s_prev[(size_t)s * A.prev_dw + k] : 0;
  }
  if (A.d_snap) {
    uint32_t* dsn = A.d_snap + (size_t)d * A.snap_dw;
    for (int k = lane; k < A.snap_dw; k += 64) dsn[k] = A.s_snap ? A.s_snap[(size_t)s * A.snap_dw + k] : 0u;
  }
}

// =========================================================================================
// host-side launchers
// =========================================================================================
hipError_t launch_import(const Variant& v, const ImportArgs& a, hipStream_t s) {
  return dispatch(v, [&](auto P, auto S) { return launch_waves(import_kernel<P, S>, a.n, s, a); });
}
hipError_t launch_export(const Variant& v, const ExportArgs& a, hipStream_t s) {
  return dispatch(v, [&](auto P, auto S) { return launch_waves(export_kernel<P, S>, a.n, s, a); });
}
hipError_t launch_records(const Variant& v, const RecordArgs& a, bool import, hipStream_t s) {
  return dispatch(v, [&](auto P, auto S) {
    if (import) return launch_waves(records_kernel<P, S, true>, a.n, s, a);
    return launch_waves(records_kernel<P, S, false>, a.n, s, a);
  });
}
hipError_t launch_copy_envs(const CopyArgs& a, hipStream_t s) {
  if (a.row_dw % 4 != 0 || a.army_dw % 8 != 0) return hipErrorInvalidValue;
  return launch_waves(copy_envs_kernel, a.n, s, a);
}

}  // namespace gvec
