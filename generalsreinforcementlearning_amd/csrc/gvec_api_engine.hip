// gvec_api_engine.hip — the engine's entry points: reset and map generation, step, legal masks, rollouts, the on-device
// agent and bot, counters.  Host only (gvec_handle.hpp); the kernels are in gvec_kernels.hip and gvec_mapgen.hip.
#include "gvec_handle.hpp"

namespace sharded {

static int32_t reset(gvec_handle* h, const int32_t* env_ids, int32_t n, const int32_t* army, const int8_t* owner, const uint8_t* type,
                     const int32_t* width, const int32_t* height, const int32_t* players, int32_t mem) {
  RET_IF(host_only(mem, "gvec_reset"));
  const size_t st = (size_t)h->stride;
  if (!env_ids) {
    return fan_range(h, 0, n, [=](gvec_handle* c, int lb, int cnt, size_t skip) {
      return gvec_reset(c, nullptr, cnt, army + skip * st, owner + skip * st, type + skip * st, width + skip, height + skip, players + skip, GVEC_MEM_HOST);
    });
  }
  // explicit ids: every shard gets the rows addressed to it, in the caller's order
  struct Part {
    std::vector<int32_t> ids, w, hh, p, army;
    std::vector<int8_t> owner;
    std::vector<uint8_t> type;
  };
  auto parts = std::make_shared<std::vector<Part>>(h->shards.size());
  for (int i = 0; i < n; ++i) {
    const int e = env_ids[i];
    if (e < 0 || e >= h->cfg.num_envs) return GVEC_E_RANGE;
    size_t k = 0;
    while (e >= h->shards[k]->begin + h->shards[k]->n) ++k;
    Part& P = (*parts)[k];
    P.ids.push_back(e - h->shards[k]->begin);
    P.w.push_back(width[i]);
    P.hh.push_back(height[i]);
    P.p.push_back(players[i]);
    P.army.insert(P.army.end(), army + i * st, army + (i + 1) * st);
    P.owner.insert(P.owner.end(), owner + i * st, owner + (i + 1) * st);
    P.type.insert(P.type.end(), type + i * st, type + (i + 1) * st);
  }
  return fan(h, [parts, h](gvec_handle* c, int begin, int) -> int32_t {
    const Part& P = (*parts)[ordinal_of(h, begin)];
    if (P.ids.empty()) return GVEC_OK;
    return gvec_reset(c, P.ids.data(), (int32_t)P.ids.size(), P.army.data(), P.owner.data(), P.type.data(), P.w.data(), P.hh.data(), P.p.data(),
                      GVEC_MEM_HOST);
  });
}

}  // namespace sharded

// f(child, the child's stats) on every shard, and the sum of what they counted in *out (null: nobody counts)
template <typename F>
static int32_t fan_stats(gvec_handle* h, gvec_rollout_stats* out, F f) {
  auto per = std::make_shared<std::vector<gvec_rollout_stats>>(h->shards.size());
  const int32_t rc = sharded::fan(h, [=](gvec_handle* c, int begin, int) { return f(c, out ? &(*per)[sharded::ordinal_of(h, begin)] : nullptr); });
  if (out) {
    memset(out, 0, sizeof *out);
    for (const gvec_rollout_stats& p : *per) {
      out->env_steps += p.env_steps;
      out->aborted_turns += p.aborted_turns;
      out->games_finished += p.games_finished;
    }
  }
  return rc;
}

// `count` generated boards into the given arrays, through the staging of the call that `st` belongs to
static int32_t generate_into(gvec_handle* h, Stage& st, uint32_t* hdr, uint32_t* rows, uint32_t* army16, int32_t* army32, int count, uint64_t seed,
                             const int32_t* width, const int32_t* height, const int32_t* players, int index_base = 0,
                             const int64_t* go_seeds = nullptr) {
  // Go-seeded boards carry a 607-word generator state each while they are being made: smaller chunks (80 MB of scratch)
  const int chunk = go_seeds ? 16384 : 65536;
  DevBuf &b_army = st.next(), &b_owner = st.next(), &b_type = st.next(), &b_w = st.next(), &b_h = st.next(), &b_p = st.next();
  DevBuf &b_iw = st.next(), &b_ih = st.next(), &b_ip = st.next(), &b_gs = st.next(), &b_gst = st.next();
  const int cn = count < chunk ? count : chunk;
  STAGE_ALLOC(b_army, (size_t)cn * h->stride * 4);
  STAGE_ALLOC(b_owner, (size_t)cn * h->stride);
  STAGE_ALLOC(b_type, (size_t)cn * h->stride);
  STAGE_ALLOC(b_w, (size_t)cn * 4);
  STAGE_ALLOC(b_h, (size_t)cn * 4);
  STAGE_ALLOC(b_p, (size_t)cn * 4);
  if (width) STAGE_ALLOC(b_iw, (size_t)cn * 4);
  if (height) STAGE_ALLOC(b_ih, (size_t)cn * 4);
  if (players) STAGE_ALLOC(b_ip, (size_t)cn * 4);
  if (go_seeds) {
    STAGE_ALLOC(b_gs, (size_t)cn * 8);
    STAGE_ALLOC(b_gst, (size_t)cn * 607 * 8);
  }
  for (int first = 0; first < count; first += chunk) {
    const int n = (count - first) < chunk ? (count - first) : chunk;
    if (width) HIPCHK(hipMemcpyAsync(b_iw.p, width + first, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    if (height) HIPCHK(hipMemcpyAsync(b_ih.p, height + first, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    if (players) HIPCHK(hipMemcpyAsync(b_ip.p, players + first, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    MapgenArgs m;
    memset(&m, 0, sizeof m);
    m.army = b_army.as<int32_t>();
    m.owner = b_owner.as<int8_t>();
    m.type = b_type.as<uint8_t>();
    m.width = b_w.as<int32_t>();
    m.height = b_h.as<int32_t>();
    m.players = b_p.as<int32_t>();
    m.in_width = width ? b_iw.as<int32_t>() : nullptr;
    m.in_height = height ? b_ih.as<int32_t>() : nullptr;
    m.in_players = players ? b_ip.as<int32_t>() : nullptr;
    m.n = n;
    m.stride = h->stride;
    m.max_w = h->cfg.max_width;
    m.max_h = h->cfg.max_height;
    m.max_p = h->maxp;
    m.first_index = index_base + first;   // board i of a shard is board env_base + i of the batch (pool boards: no offset)
    m.seed_lo = (uint32_t)seed;
    m.seed_hi = (uint32_t)(seed >> 32);
    m.status = h->d_status;
    if (go_seeds) {
      HIPCHK(hipMemcpyAsync(b_gs.p, go_seeds + first, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
      m.go_seeds = b_gs.as<int64_t>();
      m.go_state = b_gst.as<uint64_t>();
    }
    HIPCHK(launch_mapgen(m, h->stream));
    gvec_state_view v;
    memset(&v, 0, sizeof v);
    v.army = m.army;
    v.owner = m.owner;
    v.type = m.type;
    v.width = m.width;
    v.height = m.height;
    v.players = m.players;
    RET_IF(import_planes(h, hdr, rows, army16, army32, nullptr, first, n, count, &v, true, true));
    HIPCHK(hipStreamSynchronize(h->stream));  // staging is reused by the next chunk
  }
  return check_status(h, "map generation");
}

// every env a generated board: keyed by (seed, index in the batch), or board i by go_seeds[i]
static int32_t reset_generated(gvec_handle* h, uint64_t seed, const int64_t* go_seeds, const int32_t* width, const int32_t* height,
                               const int32_t* players) {
  if (h->sharded())
    return sharded::fan(h, [=](gvec_handle* c, int begin, int) {
      return reset_generated(c, seed, go_seeds ? go_seeds + begin : nullptr, width ? width + begin : nullptr, height ? height + begin : nullptr,
                             players ? players + begin : nullptr);
    });
  HIPCHK(hipSetDevice(h->cfg.device));
  Stage st(h);
  RET_IF(generate_into(h, st, h->d_hdr, h->d_rows, h->d_army16, h->d_army32, h->cfg.num_envs, seed, width, height, players,
                       go_seeds ? 0 : h->env_base, go_seeds));
  return refresh_legal(h);
}

extern "C" {

int32_t gvec_reset(gvec_handle* h, const int32_t* env_ids, int32_t n, const int32_t* army, const int8_t* owner,
                   const uint8_t* type, const int32_t* width, const int32_t* height, const int32_t* players, int32_t mem) {
  if (!h || n < 0 || !army || !owner || !type || !width || !height || !players) return GVEC_E_INVALID;
  if (n == 0) return GVEC_OK;
  if (h->sharded()) return sharded::reset(h, env_ids, n, army, owner, type, width, height, players, mem);
  if (!env_ids && n > h->cfg.num_envs) return GVEC_E_RANGE;
  if (env_ids && mem == GVEC_MEM_HOST)
    for (int i = 0; i < n; ++i)
      if (env_ids[i] < 0 || env_ids[i] >= h->cfg.num_envs) return GVEC_E_RANGE;
  HIPCHK(hipSetDevice(h->cfg.device));
  Stage st(h);
  const size_t ne = (size_t)n, nt = ne * h->stride;
  gvec_state_view v;
  memset(&v, 0, sizeof v);
  const int32_t* ids = nullptr;
  RET_IF(stage_in(h, st.next(), env_ids, ne, mem, &ids));
  RET_IF(stage_in(h, st.next(), army, nt, mem, &v.army));
  RET_IF(stage_in(h, st.next(), owner, nt, mem, &v.owner));
  RET_IF(stage_in(h, st.next(), type, nt, mem, &v.type));
  RET_IF(stage_in(h, st.next(), width, ne, mem, &v.width));
  RET_IF(stage_in(h, st.next(), height, ne, mem, &v.height));
  RET_IF(stage_in(h, st.next(), players, ne, mem, &v.players));
  RET_IF(import_planes(h, h->d_hdr, h->d_rows, h->d_army16, h->d_army32, ids, 0, n, h->cfg.num_envs, &v, true, true));
  RET_IF(check_status(h, "gvec_reset"));
  return refresh_legal(h);
}

int32_t gvec_reset_generated(gvec_handle* h, uint64_t seed, const int32_t* width, const int32_t* height,
                             const int32_t* players) {
  return h ? reset_generated(h, seed, nullptr, width, height, players) : GVEC_E_INVALID;
}

int32_t gvec_reset_go_seeded(gvec_handle* h, const int64_t* seeds, const int32_t* width, const int32_t* height, const int32_t* players) {
  return h && seeds ? reset_generated(h, 0, seeds, width, height, players) : GVEC_E_INVALID;
}

int32_t gvec_build_board_pool(gvec_handle* h, int32_t pool_size, uint64_t seed, const int32_t* width, const int32_t* height,
                              const int32_t* players) {
  if (!h || pool_size < 1) return GVEC_E_INVALID;
  if (h->sharded()) {  // every shard keeps its own copy of the same pool (board j is keyed by (seed, j) alone)
    const int32_t rc = sharded::fan(h, [=](gvec_handle* c, int, int) { return gvec_build_board_pool(c, pool_size, seed, width, height, players); });
    if (rc == GVEC_OK) h->pool_size = pool_size;
    return rc;
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (void* p : {(void*)h->p_hdr, (void*)h->p_rows, (void*)h->p_army16, (void*)h->p_army32})
    if (p) (void)hipFree(p);
  h->p_hdr = h->p_rows = h->p_army16 = nullptr;
  h->p_army32 = nullptr;
  h->pool_size = 0;
  HIPCHK(hipMalloc(&h->p_hdr, (size_t)pool_size * HDR_DW * 4));
  HIPCHK(hipMalloc(&h->p_rows, (size_t)pool_size * h->row_dw * 4));
  HIPCHK(hipMalloc(&h->p_army16, (size_t)pool_size * h->army_dw * 2));
  HIPCHK(hipMalloc(&h->p_army32, (size_t)pool_size * h->army_dw * 4));
  Stage st(h);
  RET_IF(generate_into(h, st, h->p_hdr, h->p_rows, h->p_army16, h->p_army32, pool_size, seed, width, height, players));
  h->pool_size = pool_size;
  h->pool_seed = seed;
  return GVEC_OK;
}

int32_t gvec_step(gvec_handle* h, const gvec_action* actions, int32_t* err, uint8_t* legal_bits, int32_t mem) {
  if (!h || !actions) return GVEC_E_INVALID;
  if (h->sharded()) {
    const size_t mp = (size_t)h->maxp, mb = (size_t)h->maxp * h->mask_bytes;
    return sharded::fan_host(h, mem, "gvec_step", [=](gvec_handle* c, int begin, int) {
      return gvec_step(c, actions + begin * mp, err ? err + begin : nullptr, legal_bits ? legal_bits + begin * mb : nullptr, GVEC_MEM_HOST);
    });
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t B = (size_t)h->cfg.num_envs;
  StepArgs a = base_args(h);
  if (mem == GVEC_MEM_HOST) {
    HIPCHK(hipMemcpyAsync(h->d_actions, actions, B * h->maxp * sizeof(gvec_action), hipMemcpyHostToDevice, h->stream));
    a.actions = h->d_actions;
    a.err = err ? h->d_err : nullptr;
  } else {
    a.actions = actions;
    a.err = err;
  }
  if (legal_bits) {
    // envs that sit the call out (GVEC_ACT_SKIP_ENV) or are frozen write no masks: the buffer must
    // already describe them
    if (!h->legal_valid) RET_IF(refresh_legal(h));
    a.flags |= KF_EMIT | KF_LMVALID;
  }
  HIPCHK(launch_step(h->var, a, h->stream));
  h->legal_valid = legal_bits != nullptr;
  if (mem == GVEC_MEM_HOST) {
    if (err) HIPCHK(hipMemcpyAsync(err, h->d_err, B * 4, hipMemcpyDeviceToHost, h->stream));
    if (legal_bits) HIPCHK(hipMemcpyAsync(legal_bits, h->d_legal, B * h->maxp * h->mask_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  } else if (legal_bits && legal_bits != reinterpret_cast<uint8_t*>(h->d_legal)) {
    HIPCHK(hipMemcpyAsync(legal_bits, h->d_legal, B * h->maxp * h->mask_bytes, hipMemcpyDeviceToDevice, h->stream));
  }
  return GVEC_OK;
}

int32_t gvec_legal_mask(gvec_handle* h, uint8_t* legal_bits, int32_t mem) {
  if (!h || !legal_bits) return GVEC_E_INVALID;
  if (h->sharded()) {
    const size_t mb = (size_t)h->maxp * h->mask_bytes;
    return sharded::fan_host(h, mem, "gvec_legal_mask",
                             [=](gvec_handle* c, int begin, int) { return gvec_legal_mask(c, legal_bits + begin * mb, GVEC_MEM_HOST); });
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  if (!h->legal_valid) RET_IF(refresh_legal(h));
  const size_t bytes = (size_t)h->cfg.num_envs * h->maxp * h->mask_bytes;
  if (mem == GVEC_MEM_HOST) {
    HIPCHK(hipMemcpyAsync(legal_bits, h->d_legal, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  } else if (legal_bits != reinterpret_cast<uint8_t*>(h->d_legal)) {
    HIPCHK(hipMemcpyAsync(legal_bits, h->d_legal, bytes, hipMemcpyDeviceToDevice, h->stream));
  }
  return GVEC_OK;
}

int32_t gvec_rollout(gvec_handle* h, int32_t turns, uint64_t seed, int32_t invalid_permille, int32_t fused,
                     gvec_rollout_stats* stats) {
  if (!h || turns < 0) return GVEC_E_INVALID;
  if (h->sharded())
    return fan_stats(h, stats, [=](gvec_handle* c, gvec_rollout_stats* s) { return gvec_rollout(c, turns, seed, invalid_permille, fused, s); });
  HIPCHK(hipSetDevice(h->cfg.device));
  if (stats) {
    HIPCHK(hipMemsetAsync(h->d_counters, 0, 6 * sizeof(unsigned long long), h->stream));
    HIPCHK(launch_counter_sum(h->d_hdr, h->cfg.num_envs, h->d_counters, h->stream));
  }
  StepArgs a = base_args(h);
  a.flags |= KF_AGENT | KF_EMIT;
  set_agent_seed(&a, seed, invalid_permille);
  if (fused) {
    a.turns = turns;
    if (turns > 0) HIPCHK(launch_rollout(h->var, a, h->stream));
  } else if (turns > 0) {
    if (!h->legal_valid) RET_IF(refresh_legal(h));  // the per-turn agent samples from the mask buffer
    a.turns = 1;
    a.flags |= KF_LMVALID;
    if (h->record_actions) {  // gvec_record_agent_actions: what the agent played, and what the engine said to it
      a.actions_out = h->d_actions;
      a.err = h->d_err;
    }
    for (int k = 0; k < turns; ++k) HIPCHK(launch_step(h->var, a, h->stream));
  }
  if (turns > 0) h->legal_valid = true;
  if (stats) {
    HIPCHK(launch_counter_sum(h->d_hdr, h->cfg.num_envs, h->d_counters + 3, h->stream));
    unsigned long long c[6];
    HIPCHK(hipMemcpyAsync(c, h->d_counters, sizeof c, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    stats->env_steps = (int64_t)(c[3] - c[0]);
    stats->aborted_turns = (int64_t)(c[4] - c[1]);
    stats->games_finished = (int64_t)(c[5] - c[2]);
    stats->reserved = 0;
  }
  return GVEC_OK;
}

int32_t gvec_rollout_range(gvec_handle* h, int32_t env_begin, int32_t n, int32_t turns, uint64_t seed, int32_t invalid_permille) {
  if (!h || turns < 0) return GVEC_E_INVALID;
  if (h->sharded()) return sharded::unsupported("gvec_rollout_range");
  if (!in_range(h, env_begin, n)) return GVEC_E_RANGE;
  if (n == 0 || turns == 0) return GVEC_OK;
  HIPCHK(hipSetDevice(h->cfg.device));
  if (!h->legal_valid) RET_IF(refresh_legal(h));
  // the same launch as gvec_rollout's per-turn path over a slice: every per-env array starts at the slice, and the slice's
  // first env keeps its index in the batch for the agent / pool keys (env_base)
  StepArgs a = base_args(h);
  a.flags |= KF_AGENT | KF_EMIT | KF_LMVALID;
  set_agent_seed(&a, seed, invalid_permille);
  a.turns = 1;
  const size_t e = (size_t)env_begin;
  a.hdr += e * HDR_DW;
  a.rows += e * h->row_dw;
  a.army16 += e * (h->army_dw / 2);
  a.army32 += e * h->army_dw;
  a.legal += e * h->maxp * h->mask_dw;
  a.num_envs = n;
  a.env_base = h->env_base + env_begin;
  if (h->record_actions) {
    a.actions_out = h->d_actions + e * h->maxp;
    a.err = h->d_err + e;
  }
  for (int k = 0; k < turns; ++k) HIPCHK(launch_step(h->var, a, h->stream));
  return GVEC_OK;
}

int32_t gvec_set_agent_mix(gvec_handle* h, int32_t noop_per_65536, int32_t half_per_65536) {
  if (!h) return GVEC_E_INVALID;
  if (h->sharded()) {
    for (auto& w : h->shards) RET_IF(gvec_set_agent_mix(w->h, noop_per_65536, half_per_65536));  // host-side fields only
    return GVEC_OK;
  }
  if (noop_per_65536 < 0 || noop_per_65536 > 65536 || half_per_65536 < 0 || half_per_65536 > 65536) {
    set_err("gvec_set_agent_mix: thresholds must be in [0, 65536]");
    return GVEC_E_INVALID;
  }
  h->agent_noop = (uint32_t)noop_per_65536;
  h->agent_half = (uint32_t)half_per_65536;
  return GVEC_OK;
}

int32_t gvec_record_agent_actions(gvec_handle* h, int32_t on) {
  if (!h) return GVEC_E_INVALID;
  if (h->sharded()) {
    for (auto& w : h->shards) RET_IF(gvec_record_agent_actions(w->h, on));
    return GVEC_OK;
  }
  h->record_actions = on != 0;
  return GVEC_OK;
}

int32_t gvec_counters(gvec_handle* h, gvec_rollout_stats* out) {
  if (!h || !out) return GVEC_E_INVALID;
  if (h->sharded()) return fan_stats(h, out, [](gvec_handle* c, gvec_rollout_stats* s) { return gvec_counters(c, s); });
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipMemsetAsync(h->d_counters, 0, 3 * sizeof(unsigned long long), h->stream));
  HIPCHK(launch_counter_sum(h->d_hdr, h->cfg.num_envs, h->d_counters, h->stream));
  unsigned long long c[3];
  HIPCHK(hipMemcpyAsync(c, h->d_counters, sizeof c, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  out->env_steps = (int64_t)c[0];
  out->aborted_turns = (int64_t)c[1];
  out->games_finished = (int64_t)c[2];
  out->reserved = 0;
  return GVEC_OK;
}

int32_t gvec_step_traffic_bytes(const gvec_handle* h, int64_t* out4) {
  if (!h || !out4) return GVEC_E_INVALID;
  static_assert(Planes<4>::MUTABLE == 2 * 4 + 3 && Planes<4>::LST - Planes<4>::MUTABLE == 10 && Planes<4>::COUNT - Planes<4>::LST == 4,
                "gvec_step_traffic_bytes restates the plane block's partition");
  const int64_t fd = h->fd, mp = h->var.maxp;
  const int nslot = h->var.nslot;
  const bool odd = fd == 2 * nslot - 1;
  const int64_t hdr = HDR_DW * 4;
  const int64_t mut = (2 * mp + 3) * fd * 4;    // Planes<MAXP>::MUTABLE: own, vis, chg, vch, gt1
  // gen, city, mtn, valid, ncol0, ncolL, and ok[4] where the kernel does not rebuild them (gvec_device.hpp "GVEC_LEAN")
  const int64_t cst = (lean_derive_ok(nslot) ? 6 : 10) * fd * 4;
  const int64_t lst = mp * fd * 4;              // OwnedTiles planes: only while HF_LDIFF
  const int64_t a16 = (int64_t)h->army_dw * 2, a32 = (int64_t)h->army_dw * 4;
  out4[0] = hdr + mut + cst + a16 - (lean_half_last(nslot, odd) ? 64 : 0);       // the dead half of an odd last army slot is not read
  out4[1] = hdr + mut + lean_fold_dwords((int)(2 * mp + 3), (int)fd) * 4 + a16;  // the staged store ends on a whole chunk
  out4[2] = (int64_t)h->maxp * h->mask_bytes;
  out4[3] = 2 * lst + 2 * a32;
  return GVEC_OK;
}

int32_t gvec_agent_actions(gvec_handle* h, uint64_t seed, int32_t invalid_permille, gvec_action* actions, int32_t mem) {
  if (!h || !actions) return GVEC_E_INVALID;
  if (h->sharded()) {
    const size_t mp = (size_t)h->maxp;
    return sharded::fan_host(h, mem, "gvec_agent_actions", [=](gvec_handle* c, int begin, int) {
      return gvec_agent_actions(c, seed, invalid_permille, actions + begin * mp, GVEC_MEM_HOST);
    });
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  StepArgs a = base_args(h);
  set_agent_seed(&a, seed, invalid_permille);
  a.actions_out = (mem == GVEC_MEM_HOST) ? h->d_actions : actions;
  HIPCHK(launch_agent(h->var, a, h->stream));
  if (mem == GVEC_MEM_HOST) {
    HIPCHK(hipMemcpyAsync(actions, h->d_actions, (size_t)h->cfg.num_envs * h->maxp * sizeof(gvec_action), hipMemcpyDeviceToHost,
                          h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return GVEC_OK;
}

int32_t gvec_bot_actions(gvec_handle* h, uint32_t players, uint64_t seed, int32_t random_permille, gvec_action* actions, int32_t mem) {
  if (!h || !actions) return GVEC_E_INVALID;
  if (random_permille < 0 || random_permille > 1000) {
    set_err("gvec_bot_actions: random_permille must be in [0, 1000]");
    return GVEC_E_INVALID;
  }
  if (h->maxp < 32 && (players >> h->maxp) != 0u) {
    set_err("gvec_bot_actions: players names a seat at or above max_players");
    return GVEC_E_INVALID;
  }
  if (h->sharded()) {
    const size_t mp = (size_t)h->maxp;
    return sharded::fan_host(h, mem, "gvec_bot_actions", [=](gvec_handle* c, int begin, int) {
      return gvec_bot_actions(c, players, seed, random_permille, actions + begin * mp, GVEC_MEM_HOST);
    });
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  StepArgs a = base_args(h);
  set_agent_seed(&a, seed, 0);
  const size_t bytes = (size_t)h->cfg.num_envs * h->maxp * sizeof(gvec_action);
  // host memory: the caller's array goes through the staging buffer both ways, so the slots the kernel leaves alone come
  // back as they were
  if (mem == GVEC_MEM_HOST) HIPCHK(hipMemcpyAsync(h->d_actions, actions, bytes, hipMemcpyHostToDevice, h->stream));
  a.actions_out = (mem == GVEC_MEM_HOST) ? h->d_actions : actions;
  BotArgs g;
  g.players = players;
  g.random_permille = random_permille;
  HIPCHK(launch_bot(h->var, a, g, h->stream));
  if (mem == GVEC_MEM_HOST) {
    HIPCHK(hipMemcpyAsync(actions, h->d_actions, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return GVEC_OK;
}

}  // extern "C"

// The checks of gvec_search_args that both search entry points make, under the caller's name: the arguments first, the handle
// last, so that every check of a field holds without a device.  `tail` is the caller's own checks of its further
// arguments, made after the struct's and before the handle; it sets the message itself.
template <typename Tail>
static int32_t search_check(const char* fn, gvec_handle* h, const gvec_search_args* args, Tail tail) {
  if (!args) {
    set_err("%s: args is NULL", fn);
    return GVEC_E_INVALID;
  }
  const struct {
    const void* p;
    const char* name;
  } required[] = {{args->root_players, "root_players"}, {args->candidates, "candidates"}, {args->terms, "terms"}};
  for (const auto& r : required)
    if (!r.p) {
      set_err("%s: %s is NULL", fn, r.name);
      return GVEC_E_INVALID;
    }
  if (args->num_roots < 0) {
    set_err("%s: num_roots %d is negative", fn, args->num_roots);
    return GVEC_E_INVALID;
  }
  const struct {
    int32_t v;
    const char* name;
  } counts[] = {{args->num_candidates, "num_candidates"}, {args->replicas, "replicas"}, {args->depth, "depth"}};
  for (const auto& c : counts)
    if (c.v < 1) {
      set_err("%s: %s %d is below 1", fn, c.name, c.v);
      return GVEC_E_INVALID;
    }
  // n * K * R < 2^31, without overflowing on the way
  const long long kr = (long long)args->num_candidates * args->replicas;
  if (kr >= (1ll << 31) || (long long)args->num_roots * kr >= (1ll << 31)) {
    set_err("%s: num_roots * num_candidates * replicas = %d * %d * %d playouts is not below 2^31", fn, args->num_roots, args->num_candidates,
            args->replicas);
    return GVEC_E_INVALID;
  }
  if (const int32_t rc = tail()) return rc;
  if (!h) {
    set_err("%s: h is NULL", fn);
    return GVEC_E_INVALID;
  }
  return GVEC_OK;
}

// the launch arguments of a checked call on an unsharded handle
static void search_launch_args(gvec_handle* h, const gvec_search_args* args, StepArgs& a, SearchArgs& g) {
  a = base_args(h);
  a.flags = KF_AGENT;   // no re-deal, no mask emission: the kernel writes terms alone
  set_agent_seed(&a, args->seed, 0);
  g.root_envs = args->root_envs;
  g.root_players = args->root_players;
  g.candidates = args->candidates;
  g.terms = args->terms;
  g.num_candidates = args->num_candidates;
  g.replicas = args->replicas;
  g.depth = args->depth;
  g.num_playouts = (int32_t)((long long)args->num_roots * args->num_candidates * args->replicas);
  g.stride = h->stride;
}

extern "C" {

int32_t gvec_search_playouts(gvec_handle* h, const gvec_search_args* args) {
  static const char* fn = "gvec_search_playouts";
  if (const int32_t rc = search_check(fn, h, args, [] { return (int32_t)GVEC_OK; })) return rc;
  if (h->sharded()) return sharded::unsupported(fn);
  if (args->num_roots == 0) return GVEC_OK;
  HIPCHK(hipSetDevice(h->cfg.device));
  StepArgs a;
  SearchArgs g;
  search_launch_args(h, args, a, g);
  HIPCHK(launch_search(h->var, a, g, h->stream));
  return GVEC_OK;
}

int32_t gvec_search_playouts_bot(gvec_handle* h, const gvec_search_args* args, uint32_t bot_players, int32_t bot_random_permille) {
  static const char* fn = "gvec_search_playouts_bot";
  // gvec_bot_actions' two checks in its wording; the seat mask against the largest handle first, which needs no handle
  const auto seats_above = [&](int maxp) {
    if (maxp >= 32 || (bot_players >> maxp) == 0u) return (int32_t)GVEC_OK;
    set_err("%s: bot_players names a seat at or above max_players", fn);
    return (int32_t)GVEC_E_INVALID;
  };
  const auto tail = [&] {
    if (bot_random_permille < 0 || bot_random_permille > 1000) {
      set_err("%s: bot_random_permille must be in [0, 1000]", fn);
      return (int32_t)GVEC_E_INVALID;
    }
    return seats_above(GVEC_MAX_PLAYERS);
  };
  if (const int32_t rc = search_check(fn, h, args, tail)) return rc;
  if (const int32_t rc = seats_above(h->maxp)) return rc;
  if (h->sharded()) return sharded::unsupported(fn);
  if (args->num_roots == 0) return GVEC_OK;
  HIPCHK(hipSetDevice(h->cfg.device));
  StepArgs a;
  SearchArgs g;
  search_launch_args(h, args, a, g);
  BotArgs bot;
  bot.players = bot_players;
  bot.random_permille = bot_random_permille;
  HIPCHK(launch_search_bot(h->var, a, g, bot, h->stream));
  return GVEC_OK;
}

int32_t gvec_search_expand(gvec_handle* h, const gvec_search_args* args, uint32_t bot_players, int32_t bot_random_permille, gvec_handle* dst,
                           const int32_t* child_envs, int32_t* status) {
  static const char* fn = "gvec_search_expand";
  const auto seats_above = [&](int maxp) {
    if (maxp >= 32 || (bot_players >> maxp) == 0u) return (int32_t)GVEC_OK;
    set_err("%s: bot_players names a seat at or above max_players", fn);
    return (int32_t)GVEC_E_INVALID;
  };
  const auto tail = [&] {
    if (bot_random_permille < 0 || bot_random_permille > 1000) {
      set_err("%s: bot_random_permille must be in [0, 1000]", fn);
      return (int32_t)GVEC_E_INVALID;
    }
    return seats_above(GVEC_MAX_PLAYERS);
  };
  if (const int32_t rc = search_check(fn, h, args, tail)) return rc;
  if (const int32_t rc = seats_above(h->maxp)) return rc;
  if (h->sharded() || (dst && dst->sharded())) return sharded::unsupported(fn);
  if (dst) {   // what gvec_copy_envs asks of a pair of handles: the same variant, plane stride, army block and rules
    const gvec_config &dc = dst->cfg, &sc = h->cfg;
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
      set_err("%s: the handles differ in %s", fn, field);
      return GVEC_E_INVALID;
    }
  }
  if (args->num_roots == 0) return GVEC_OK;
  HIPCHK(hipSetDevice(h->cfg.device));
  StepArgs a;
  SearchArgs g;
  search_launch_args(h, args, a, g);
  SearchKeepArgs e;
  memset(&e, 0, sizeof e);
  e.child_envs = child_envs;
  e.status = status;
  if (dst) {
    e.hdr = dst->d_hdr;
    e.rows = dst->d_rows;
    e.army16 = dst->d_army16;
    e.army32 = dst->d_army32;
    e.num_envs = dst->cfg.num_envs;
  }
  // ordered after the work already enqueued on dst's stream; dst's next call waits for the launch in turn
  const bool cross = dst && dst != h && dst->stream != h->stream;
  hipEvent_t ev = nullptr;
  if (cross) {
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t w = hipEventRecord(ev, dst->stream);
    if (w == hipSuccess) w = hipStreamWaitEvent(h->stream, ev, 0);
    if (w != hipSuccess) {
      (void)hipEventDestroy(ev);
      HIPCHK(w);
    }
  }
  hipError_t rc;
  if (bot_players == 0u && bot_random_permille == 0) {
    rc = launch_search_expand(h->var, a, g, e, h->stream);
  } else {
    BotArgs bot;
    bot.players = bot_players;
    bot.random_permille = bot_random_permille;
    rc = launch_search_expand_bot(h->var, a, g, bot, e, h->stream);
  }
  if (cross) {
    if (rc == hipSuccess) rc = hipEventRecord(ev, h->stream);
    if (rc == hipSuccess) rc = hipStreamWaitEvent(dst->stream, ev, 0);
    (void)hipEventDestroy(ev);  // released once the recorded work completes
  }
  HIPCHK(rc);
  if (dst) dst->legal_valid = false;   // the per-turn agent samples from d_legal: the stored envs' rows of it are stale
  return GVEC_OK;
}

}  // extern "C"
