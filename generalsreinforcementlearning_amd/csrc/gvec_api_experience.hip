// gvec_api_experience.hip — what a learner reads off a handle: experience snapshots, rewards and records (and their
// expansion), observations, the serializer's mask and the experience stream's deltas.  Host only (gvec_handle.hpp); the
// kernels are in gvec_experience.hip and gvec_stream.hip.
#include <cmath>

#include "gvec_handle.hpp"

static ExperienceArgs exp_args(gvec_handle* h) {
  ExperienceArgs a = state_args<ExperienceArgs>(h);
  a.snap = h->d_snap;
  a.num_envs = h->cfg.num_envs;
  a.fd = h->fd;
  a.row_dw = h->row_dw;
  a.snap_dw = h->snap_dw;
  a.record_dw = h->record_dw;
  a.pstride = h->maxp;
  a.stride = h->stride;
  a.player = -1;
  return a;
}

int32_t ensure_snapshots(gvec_handle* h) {
  if (!h->d_snap) {
    experience_layout(h->var, h->fd, &h->snap_dw, &h->record_dw);
    HIPCHK(hipMalloc(&h->d_snap, (size_t)h->cfg.num_envs * h->snap_dw * 4));
    HIPCHK(hipMemset(h->d_snap, 0, (size_t)h->cfg.num_envs * h->snap_dw * 4));
  }
  return GVEC_OK;
}

static StreamDeltaArgs stream_args(gvec_handle* h, int32_t player, int cap) {
  StreamDeltaArgs a = state_args<StreamDeltaArgs>(h);
  a.num_envs = h->cfg.num_envs;
  a.fd = h->fd;
  a.row_dw = h->row_dw;
  a.player = player;
  a.cap = cap;
  return a;
}

namespace sharded {

static int32_t gather_records(gvec_handle* h, int32_t local_begin, int32_t n, int32_t env_id_base, int32_t mem, int32_t dst_device, void* dst) {
  if (!dst || n < 0 || local_begin < 0) return GVEC_E_INVALID;
  for (auto& w : h->shards)
    if (local_begin + n > w->n) {
      set_err("gvec_gather_experience_records: envs [%d, %d) of every shard, but a shard holds %d", local_begin, local_begin + n, w->n);
      return GVEC_E_RANGE;
    }
  if (n == 0) return GVEC_OK;
  const size_t rec = (size_t)gvec_experience_record_bytes(h);
  return fan(h, [=](gvec_handle* c, int begin, int) -> int32_t {
    HIPCHK(hipSetDevice(c->cfg.device));
    DevBuf stage = Stage::reserved(c);   // alive across gvec_experience_records, whose own staging starts at slot 0
    STAGE_ALLOC(stage, (size_t)n * rec);
    RET_IF(gvec_experience_records(c, nullptr, GVEC_MEM_DEVICE, local_begin, n, env_id_base + begin, stage.p));
    char* to = reinterpret_cast<char*>(dst) + (size_t)ordinal_of(h, begin) * n * rec;
    if (mem == GVEC_MEM_HOST) HIPCHK(hipMemcpyAsync(to, stage.p, (size_t)n * rec, hipMemcpyDeviceToHost, c->stream));
    else if (dst_device == c->cfg.device) HIPCHK(hipMemcpyAsync(to, stage.p, (size_t)n * rec, hipMemcpyDeviceToDevice, c->stream));
    else HIPCHK(hipMemcpyPeerAsync(to, dst_device, stage.p, c->cfg.device, (size_t)n * rec, c->stream));   // over xGMI
    HIPCHK(hipStreamSynchronize(c->stream));
    return GVEC_OK;
  });
}

}  // namespace sharded

extern "C" {

int32_t gvec_experience_begin_range(gvec_handle* h, int32_t env_begin, int32_t n) {
  if (!h) return GVEC_E_INVALID;
  if (h->sharded())
    return sharded::fan_range(h, env_begin, n, [](gvec_handle* c, int lb, int cnt, size_t) { return gvec_experience_begin_range(c, lb, cnt); });
  if (!in_range(h, env_begin, n)) return GVEC_E_RANGE;
  if (n == 0) return GVEC_OK;
  HIPCHK(hipSetDevice(h->cfg.device));
  RET_IF(ensure_snapshots(h));
  ExperienceArgs a = exp_args(h);
  a.env_begin = env_begin;
  a.num_envs = n;
  HIPCHK(launch_snapshot(h->var, a, h->stream));
  return GVEC_OK;
}

int32_t gvec_experience_begin(gvec_handle* h) { return h ? gvec_experience_begin_range(h, 0, h->cfg.num_envs) : GVEC_E_INVALID; }

int32_t gvec_experience_rewards(gvec_handle* h, float* rewards, uint8_t* done, int32_t mem) {
  if (!h || !rewards) return GVEC_E_INVALID;
  if (h->sharded()) {
    const size_t mp = (size_t)h->maxp;
    return sharded::fan_host(h, mem, "gvec_experience_rewards", [=](gvec_handle* c, int begin, int) {
      return gvec_experience_rewards(c, rewards + begin * mp, done ? done + begin : nullptr, GVEC_MEM_HOST);
    });
  }
  if (!h->d_snap) {
    set_err("gvec_experience_rewards without a preceding gvec_experience_begin");
    return GVEC_E_INVALID;
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t B = (size_t)h->cfg.num_envs;
  Stage st(h);
  DevBuf &br = st.next(), &bd = st.next();
  ExperienceArgs a = exp_args(h);
  RET_IF(stage_out(br, rewards, B * h->maxp, mem, &a.rewards));
  RET_IF(stage_out(bd, done, B, mem, &a.done));
  HIPCHK(launch_rewards(h->var, a, h->stream));
  RET_IF(copy_out(h, br, rewards, B * h->maxp, mem));
  RET_IF(copy_out(h, bd, done, B, mem));
  if (mem == GVEC_MEM_HOST) HIPCHK(hipStreamSynchronize(h->stream));
  return GVEC_OK;
}

int32_t gvec_reward_config_default(gvec_reward_config* cfg) {
  if (!cfg) return null_args("gvec_reward_config_default");
  *cfg = gvec_reward_config{};
  cfg->win_game = 1.0f;           // DefaultRewardConfig, rewards.go:23-37
  cfg->lose_game = -1.0f;
  cfg->capture_city = 0.1f;
  cfg->lose_city = -0.1f;
  cfg->capture_general = 0.5f;
  cfg->lose_general = -0.5f;
  cfg->territory = 0.01f;         // TerritoryGained (TerritoryLost is never read)
  cfg->army = 0.001f;             // ArmyGained (ArmyLost is never read)
  cfg->army_advantage = 0.05f;
  return GVEC_OK;
}

int32_t gvec_experience_begin_rewards(gvec_handle* h) {
  if (!h) return null_args("gvec_experience_begin_rewards");
  if (h->sharded()) return sharded::fan(h, [](gvec_handle* c, int, int) { return gvec_experience_begin_rewards(c); });
  if (h->cfg.num_envs == 0) return GVEC_OK;
  HIPCHK(hipSetDevice(h->cfg.device));
  RET_IF(ensure_snapshots(h));
  ExperienceArgs a = exp_args(h);
  a.env_begin = 0;
  HIPCHK(launch_snapshot_rewards(h->var, a, h->stream));
  return GVEC_OK;
}

int32_t gvec_experience_rewards_config(gvec_handle* h, const gvec_reward_config* cfg, uint32_t players, const uint8_t* invalid, float* rewards,
                                       int32_t* terms, uint8_t* done, int32_t mem) {
  static const char* fn = "gvec_experience_rewards_config";
  // everything that can be said of the arguments alone comes first: it holds without a handle and without a device
  if (!cfg) {
    set_err("%s: cfg is NULL", fn);
    return GVEC_E_INVALID;
  }
  const float w[10] = {cfg->win_game, cfg->lose_game, cfg->capture_city, cfg->lose_city, cfg->capture_general, cfg->lose_general,
                       cfg->territory, cfg->army, cfg->army_advantage, cfg->invalid_action};
  static const char* names[10] = {"win_game", "lose_game", "capture_city", "lose_city", "capture_general", "lose_general",
                                  "territory", "army", "army_advantage", "invalid_action"};
  for (int k = 0; k < 10; ++k)
    if (!std::isfinite(w[k])) {
      set_err("%s: %s is not finite", fn, names[k]);
      return GVEC_E_INVALID;
    }
  if (cfg->reserved != 0u) {
    set_err("%s: reserved must be 0", fn);
    return GVEC_E_INVALID;
  }
  if (cfg->flags & ~GVEC_REWARD_CLIP) {
    set_err("%s: unknown flag bits 0x%x", fn, cfg->flags & ~GVEC_REWARD_CLIP);
    return GVEC_E_INVALID;
  }
  if (!rewards && !terms && !done) {
    set_err("%s: rewards, terms and done are all NULL", fn);
    return GVEC_E_INVALID;
  }
  if (players >> GVEC_MAX_PLAYERS) {
    set_err("%s: players 0x%x names a seat at or above GVEC_MAX_PLAYERS", fn, players);
    return GVEC_E_INVALID;
  }
  if (!h) {
    set_err("%s: the handle is NULL", fn);
    return GVEC_E_INVALID;
  }
  if (players >> h->maxp) {
    set_err("%s: players 0x%x names a seat at or above max_players = %d", fn, players, h->maxp);
    return GVEC_E_INVALID;
  }
  const uint32_t bits = players ? players : ((1u << h->maxp) - 1u);
  const size_t K = (size_t)__builtin_popcount(bits);
  if (h->sharded())
    return sharded::fan_host(h, mem, fn, [=](gvec_handle* c, int begin, int) {
      return gvec_experience_rewards_config(c, cfg, players, invalid ? invalid + begin * K : nullptr, rewards ? rewards + begin * K : nullptr,
                                            terms ? terms + begin * K * 8 : nullptr, done ? done + begin : nullptr, GVEC_MEM_HOST);
    });
  if (!h->d_snap) {
    set_err("%s without a preceding gvec_experience_begin or gvec_experience_begin_rewards", fn);
    return GVEC_E_INVALID;
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t B = (size_t)h->cfg.num_envs;
  Stage st(h);
  DevBuf &bi = st.next(), &br = st.next(), &bt = st.next(), &bd = st.next();
  RewardArgs a = state_args<RewardArgs>(h);
  a.snap = h->d_snap;
  a.cfg = *cfg;
  a.players = bits;
  a.nk = (int32_t)K;
  a.num_envs = h->cfg.num_envs;
  a.fd = h->fd;
  a.row_dw = h->row_dw;
  a.snap_dw = h->snap_dw;
  RET_IF(stage_in(h, bi, invalid, B * K, mem, &a.invalid));
  RET_IF(stage_out(br, rewards, B * K, mem, &a.rewards));
  RET_IF(stage_out(bt, terms, B * K * 8, mem, &a.terms));
  RET_IF(stage_out(bd, done, B, mem, &a.done));
  HIPCHK(launch_rewards_config(h->var, a, h->stream));
  RET_IF(copy_out(h, br, rewards, B * K, mem));
  RET_IF(copy_out(h, bt, terms, B * K * 8, mem));
  RET_IF(copy_out(h, bd, done, B, mem));
  if (mem == GVEC_MEM_HOST) HIPCHK(hipStreamSynchronize(h->stream));
  return GVEC_OK;
}

int32_t gvec_experience_record_layout(gvec_handle* h, int32_t* out8) {
  if (!h || !out8) return GVEC_E_INVALID;
  int snap_dw = 0, record_dw = 0;
  experience_layout(h->var, h->fd, &snap_dw, &record_dw);
  out8[0] = record_dw;          // dwords per record
  out8[1] = h->var.maxp;        // player slots of the layout (>= max_players)
  out8[2] = h->fd;              // dwords per bit-plane
  out8[3] = h->var.nslot;       // 64-tile army slots
  out8[4] = h->maxp;            // max_players of the handle
  out8[5] = h->stride;          // max_width * max_height
  out8[6] = 0;
  out8[7] = 0;
  return GVEC_OK;
}

int32_t gvec_experience_record_bytes(gvec_handle* h) {
  int32_t l[8];
  const int32_t rc = gvec_experience_record_layout(h, l);
  return rc < 0 ? rc : l[0] * 4;
}

int32_t gvec_experience_records(gvec_handle* h, const gvec_action* actions, int32_t mem, int32_t env_begin, int32_t n,
                                int32_t env_id_base, void* dst_device) {
  if (!h || !dst_device) return GVEC_E_INVALID;
  if (h->sharded()) return sharded::unsupported("gvec_experience_records (a sharded handle collects with gvec_gather_experience_records)");
  if (!in_range(h, env_begin, n)) return GVEC_E_RANGE;
  if (!h->d_snap) {
    set_err("gvec_experience_records without a preceding gvec_experience_begin");
    return GVEC_E_INVALID;
  }
  if (n == 0) return GVEC_OK;
  HIPCHK(hipSetDevice(h->cfg.device));
  ExperienceArgs a = exp_args(h);
  if (!actions) {
    a.actions = h->d_actions;  // the last gvec_step (host mode) / recorded device-agent turn
  } else if (mem == GVEC_MEM_HOST) {
    HIPCHK(hipMemcpyAsync(h->d_actions, actions, (size_t)h->cfg.num_envs * h->maxp * sizeof(gvec_action), hipMemcpyHostToDevice, h->stream));
    a.actions = h->d_actions;
  } else {
    a.actions = actions;
  }
  a.env_begin = env_begin;
  a.num_envs = n;
  a.env_id_base = env_id_base;
  a.records = reinterpret_cast<uint32_t*>(dst_device);
  HIPCHK(launch_experience_records(h->var, a, h->stream));
  return GVEC_OK;
}

int32_t gvec_gather_experience_records(gvec_handle* h, int32_t shard_env_begin, int32_t n, int32_t env_id_base, int32_t mem, int32_t dst_device,
                                       void* dst) {
  if (!h || !h->sharded()) {
    set_err("gvec_gather_experience_records needs a sharded handle (a plain one writes its records with gvec_experience_records)");
    return GVEC_E_INVALID;
  }
  return sharded::gather_records(h, shard_env_begin, n, env_id_base, mem, dst_device, dst);
}

int32_t gvec_expand_experience_records(int32_t device, void* hip_stream, const int32_t* layout8, const void* records, int32_t n, float* state,
                                       float* next_state, uint8_t* action_mask, int32_t* meta) {
  if (!layout8 || !records || !state || !next_state || !action_mask || !meta || n < 0) return GVEC_E_INVALID;
  const int rd = layout8[0], mp = layout8[1], fd = layout8[2], ns = layout8[3], stride = layout8[5];
  if (mp < 1 || mp > GVEC_MAX_PLAYERS || fd < 1 || fd > 32 || ns < 1 || ns > 16 || stride < 1 || stride > GVEC_MAX_DIM * GVEC_MAX_DIM ||
      stride > 32 * fd || stride > 64 * ns || rd < 4 + 2 * mp + (8 * mp + 3) * fd + ns * 64 || rd > 4 + 2 * mp + (8 * mp + 3) * fd + ns * 64 + 3) {
    set_err("gvec_expand_experience_records: layout {%d, %d, %d, %d, ., %d} is not one gvec_experience_record_layout produces", rd, mp, fd, ns, stride);
    return GVEC_E_INVALID;
  }
  // expand_records_kernel reads a record as dwords and writes a tile's four mask bytes (and an absent slot's zeros) as one
  // dword; every slot of action_mask is 4 * stride bytes, so the array's own alignment decides
  if ((reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(action_mask)) & 3u) {
    set_err("gvec_expand_experience_records: records and action_mask must be 4-byte aligned (%s is not)",
            (reinterpret_cast<uintptr_t>(records) & 3u) ? "records" : "action_mask");
    return GVEC_E_INVALID;
  }
  if (n == 0) return GVEC_OK;
  ON_DEVICE(device, launch_expand_records(records, n, layout8, state, next_state, action_mask, meta, reinterpret_cast<hipStream_t>(hip_stream)));
}

int32_t gvec_observe(gvec_handle* h, int32_t player, float* out, int32_t mem) {
  if (!h || !out || player < -1 || player >= h->maxp) return GVEC_E_INVALID;
  if (h->sharded()) {
    const size_t per = (size_t)(player < 0 ? h->maxp : 1) * 9 * h->stride;
    return sharded::fan_host(h, mem, "gvec_observe", [=](gvec_handle* c, int begin, int) { return gvec_observe(c, player, out + begin * per, GVEC_MEM_HOST); });
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t count = (size_t)h->cfg.num_envs * (player < 0 ? h->maxp : 1) * 9 * h->stride;
  Stage st(h);
  DevBuf& bo = st.next();
  ExperienceArgs a = exp_args(h);
  a.player = player;
  RET_IF(stage_out(bo, out, count, mem, &a.obs));
  HIPCHK(launch_observe(h->var, a, h->stream));
  RET_IF(copy_out(h, bo, out, count, mem));
  if (mem == GVEC_MEM_HOST) HIPCHK(hipStreamSynchronize(h->stream));
  return GVEC_OK;
}

int32_t gvec_serializer_mask(gvec_handle* h, uint8_t* bits, int32_t mem) {
  if (!h || !bits) return GVEC_E_INVALID;
  if (mem == GVEC_MEM_DEVICE && (reinterpret_cast<uintptr_t>(bits) & 3u)) {   // the kernel stores the planes as dwords
    set_err("gvec_serializer_mask: a device bits array must be 4-byte aligned");
    return GVEC_E_INVALID;
  }
  if (h->sharded()) {
    const size_t mb = (size_t)h->maxp * h->mask_bytes;
    return sharded::fan_host(h, mem, "gvec_serializer_mask", [=](gvec_handle* c, int begin, int) { return gvec_serializer_mask(c, bits + begin * mb, GVEC_MEM_HOST); });
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t bytes = (size_t)h->cfg.num_envs * h->maxp * h->mask_bytes;
  Stage st(h);
  DevBuf& bb = st.next();
  StepArgs a = base_args(h);
  uint8_t* dst = nullptr;
  RET_IF(stage_out(bb, bits, bytes, mem, &dst));
  a.legal = reinterpret_cast<uint32_t*>(dst);
  HIPCHK(launch_serializer_mask(h->var, a, h->stream));
  RET_IF(copy_out(h, bb, bits, bytes, mem));
  if (mem == GVEC_MEM_HOST) HIPCHK(hipStreamSynchronize(h->stream));
  return GVEC_OK;
}

int32_t gvec_stream_delta_cap(const gvec_handle* h) { return h ? (h->stride / 5 > 1 ? h->stride / 5 : 1) : GVEC_E_INVALID; }

int32_t gvec_stream_deltas(gvec_handle* h, int32_t player, uint8_t* kind, int32_t* count, uint64_t* updates, int32_t mem) {
  if (!h || !kind || !count || !updates || player < 0 || player >= h->maxp) return GVEC_E_INVALID;
  const int cap = gvec_stream_delta_cap(h);
  if (h->sharded())
    return sharded::fan_host(h, mem, "gvec_stream_deltas", [=](gvec_handle* c, int begin, int) {
      return gvec_stream_deltas(c, player, kind + begin, count + begin, updates + (size_t)begin * cap, GVEC_MEM_HOST);
    });
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t B = (size_t)h->cfg.num_envs;
  Stage st(h);
  DevBuf &bk = st.next(), &bc = st.next(), &bu = st.next();
  StreamDeltaArgs a = stream_args(h, player, cap);
  unsigned long long* du = nullptr;
  RET_IF(stage_out(bk, kind, B, mem, &a.kind));
  RET_IF(stage_out(bc, count, B, mem, &a.count));
  RET_IF(stage_out(bu, reinterpret_cast<unsigned long long*>(updates), B * cap, mem, &du));
  a.updates = du;
  HIPCHK(launch_stream_deltas(h->var, a, h->stream));
  RET_IF(copy_out(h, bk, kind, B, mem));
  RET_IF(copy_out(h, bc, count, B, mem));
  RET_IF(copy_out(h, bu, reinterpret_cast<unsigned long long*>(updates), B * cap, mem));
  if (mem == GVEC_MEM_HOST) HIPCHK(hipStreamSynchronize(h->stream));
  return GVEC_OK;
}

int32_t gvec_stream_deltas_packed(gvec_handle* h, int32_t player, int32_t full_tiles, uint8_t* kind, int64_t* offset, uint64_t* updates,
                                  int64_t capacity, int64_t* total) {
  if (!h || !kind || !offset || !updates || !total || capacity < 0 || player < 0 || player >= h->maxp) return GVEC_E_INVALID;
  if (h->sharded()) return sharded::unsupported("gvec_stream_deltas_packed");
  HIPCHK(hipSetDevice(h->cfg.device));
  const int cap = full_tiles ? h->stride : gvec_stream_delta_cap(h);   // rows long enough for a whole board when asked for
  const size_t B = (size_t)h->cfg.num_envs;
  Stage st(h);
  DevBuf &bk = st.next(), &bc = st.next(), &bu = st.next(), &bo = st.next(), &bp = st.next();
  STAGE_ALLOC(bk, B);
  STAGE_ALLOC(bc, B * 4);
  STAGE_ALLOC(bu, B * cap * 8);
  STAGE_ALLOC(bo, (B + 1) * 8);
  STAGE_ALLOC(bp, B * cap * 8);
  StreamDeltaArgs a = stream_args(h, player, cap);
  a.full_tiles = full_tiles ? 1 : 0;
  a.kind = bk.as<uint8_t>();
  a.count = bc.as<int32_t>();
  a.updates = bu.as<unsigned long long>();
  HIPCHK(launch_stream_deltas(h->var, a, h->stream));
  HIPCHK(launch_pack_updates(bu.as<unsigned long long>(), bc.as<int32_t>(), bo.as<long long>(), bp.as<unsigned long long>(), h->cfg.num_envs, cap,
                             (long long)(B * cap), h->stream));
  HIPCHK(hipMemcpyAsync(kind, bk.p, B, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(offset, bo.p, (B + 1) * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *total = offset[B];
  if (*total > capacity) {
    set_err("gvec_stream_deltas_packed: %lld updates, room for %lld", (long long)*total, (long long)capacity);
    return GVEC_E_RANGE;
  }
  if (*total > 0) {
    HIPCHK(hipMemcpyAsync(updates, bp.p, (size_t)*total * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return GVEC_OK;
}

}  // extern "C"
