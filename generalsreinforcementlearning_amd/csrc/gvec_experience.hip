// gvec_experience.hip — internal/experience on the device: the snapshot before a step, rewards, experience records and
// their expansion into tensors, the observation tensor.
#include "gvec_dispatch.hpp"
#include "gvec_gym_emit.hpp"
#include "gvec_turn.hpp"

namespace gvec {

// =========================================================================================
// internal/experience: snapshot (GameState.Clone before the step), rewards, observation tensor
// =========================================================================================
// Snapshot of env e (snap_dw dwords): what the reward AND the experience record need of the state before the
// step - prev own planes [MAXP][fd] | prev vis planes [MAXP][fd] | Serializer.GenerateActionMask(prev) as four
// direction planes per player [MAXP][4][fd] | prev armies as u16, tile t at halfword t, saturated to [0, 65535]
// (StateToTensor clamps army / 1000 at 1, serializer.go:82-85: saturation is exact for it) [NSLOT*32] |
// tail: territory [MAXP], armies [MAXP], turn, W | H << 8.
template <int MAXP, int NSLOT>
struct SnapLayout {
  int fd;
  __host__ __device__ int own() const { return 0; }
  __host__ __device__ int vis() const { return MAXP * fd; }
  __host__ __device__ int mask() const { return 2 * MAXP * fd; }
  __host__ __device__ int army() const { return 6 * MAXP * fd; }
  __host__ __device__ int tail() const { return 6 * MAXP * fd + NSLOT * 32; }
  __host__ __device__ int total() const { return (tail() + 2 * MAXP + 2 + 3) / 4 * 4; }
};

// Tile.Army as the u16 a tensor consumer needs: lane l of slot s is tile 64s + l
template <int NSLOT>
__device__ __forceinline__ void store_army_sat16(const int32_t (&army)[NSLOT], uint32_t* dst) {
  uint16_t* h = reinterpret_cast<uint16_t*>(dst);
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) {
    const int32_t a = army[s];
    h[64 * s + lane_id()] = (uint16_t)(a < 0 ? 0 : (a > 65535 ? 65535 : a));
  }
}

template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void snapshot_kernel(ExperienceArgs A) {
  using B = Board<MAXP, NSLOT>;
  const int lane = lane_id();
  const int i = wave_item();
  if (i >= A.num_envs) return;
  const int env = A.env_begin + i;
  B b;
  load_board(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd);
  const SnapLayout<MAXP, NSLOT> L{A.fd};
  uint32_t* sn = A.snap + (size_t)env * A.snap_dw;
  uint32_t tail = 0u;  // lane p: territory, lane MAXP+p: armies, lane 2*MAXP: turn, +1: W|H<<8
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    if (lane < A.fd) {
      sn[L.own() + p * A.fd + lane] = b.own[p];
      sn[L.vis() + p * A.fd + lane] = b.vis[p];
      // Serializer.GenerateActionMask (serializer.go:112-176): board owner, army >= 2, no Alive check;
      // d = 0 up, 1 DOWN, 2 LEFT, 3 right
      const uint32_t src = b.own[p] & b.gt1;
      uint32_t* m = sn + L.mask() + p * 4 * A.fd + lane;
      m[0 * A.fd] = src & b.ok[0];
      m[1 * A.fd] = src & b.ok[2];
      m[2 * A.fd] = src & b.ok[3];
      m[3 * A.fd] = src & b.ok[1];
    }
    const int32_t terr = b.count(b.own[p]), arm = b.army_sum(b.own[p]);
    tail = (lane == p) ? (uint32_t)terr : tail;
    tail = (lane == MAXP + p) ? (uint32_t)arm : tail;
  }
  store_army_sat16<NSLOT>(b.army, sn + L.army());
  tail = (lane == 2 * MAXP) ? (uint32_t)b.turn : tail;
  tail = (lane == 2 * MAXP + 1) ? ((uint32_t)b.W | ((uint32_t)b.H << 8)) : tail;
  if (lane < 2 * MAXP + 2) sn[L.tail() + lane] = tail;
}

// CalculateRewardWithConfig (internal/experience/rewards.go:45-85) with DefaultRewardConfig (:23-37);
// prev = the snapshot, cur = the resident state.  float32 arithmetic in the reference's order,
// compiled with -ffp-contract=off (Go on amd64 does not fuse multiply-add).  Lane p receives player p's reward.
template <int MAXP, int NSLOT>
__device__ __forceinline__ float compute_rewards(const Board<MAXP, NSLOT>& b, const uint32_t* sn, int fd, bool& over, bool& comparable) {
  const int lane = lane_id();
  const SnapLayout<MAXP, NSLOT> L{fd};
  const uint32_t tail = (lane < 2 * MAXP + 2) ? sn[L.tail() + lane] : 0u;
  const int prev_turn = (int)rdlane(tail, 2 * MAXP);
  const uint32_t prev_dims = rdlane(tail, 2 * MAXP + 1);
  // a board re-dealt by auto-reset (or not stepped) has no meaningful predecessor: reward 0
  comparable = prev_dims == ((uint32_t)b.W | ((uint32_t)b.H << 8)) && b.turn > prev_turn;
  const int na = __builtin_popcount(b.alive);
  over = na <= 1;                                                // GameState.IsGameOver (state.go:73-82)
  const int winner = (na == 1) ? (31 - __builtin_clz(b.alive)) : -1;  // GameState.GetWinner (state.go:85-100)
  uint32_t prev_own[MAXP], prev_any = 0u;
  int32_t cur_arm[MAXP], total = 0;
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    prev_own[p] = (lane < fd) ? sn[L.own() + p * fd + lane] : 0u;
    prev_any |= prev_own[p];
    cur_arm[p] = b.army_sum(b.own[p]);
    total += cur_arm[p];
  }
  float rv = 0.0f;
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    const int d_terr = b.count(b.own[p]) - (int)rdlane(tail, p);             // :59-62
    const int d_arm = cur_arm[p] - (int)rdlane(tail, MAXP + p);               // :65-68
    const int c_gain = b.count(b.city & b.own[p] & ~prev_own[p]);             // countCityChanges :110-129
    const int c_lost = b.count(b.city & prev_own[p] & ~b.own[p]);
    const int g_gain = b.count(b.gen & b.own[p] & ~prev_own[p] & prev_any);   // countGeneralChanges :132-151
    const int g_lost = b.count(b.gen & prev_own[p] & ~b.own[p]);
    float r = 0.0f;
    r += (float)d_terr * 0.01f;
    r += (float)d_arm * 0.001f;
    r += (float)c_gain * 0.1f;
    r += (float)c_lost * -0.1f;
    r += (float)g_gain * 0.5f;
    r += (float)g_lost * -0.5f;
    const int pa = cur_arm[p], ea = total - cur_arm[p];                       // calculateArmyAdvantage :153-175
    const float adv = (total == 0) ? 0.0f : ((float)(pa - ea) / (float)total);
    r += adv * 0.05f;
    if (over && winner == p) r = 1.0f;                                        // :49-56
    else if (over && winner != -1) r = -1.0f;
    r = (comparable && p < b.P) ? r : 0.0f;
    rv = (lane == p) ? r : rv;
  }
  return rv;
}

template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void rewards_kernel(ExperienceArgs A) {
  using B = Board<MAXP, NSLOT>;
  const int lane = lane_id();
  const int i = wave_item();
  if (i >= A.num_envs) return;
  const int env = A.env_begin + i;
  B b;
  load_board(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd);
  bool over, comparable;
  const float rv = compute_rewards<MAXP, NSLOT>(b, A.snap + (size_t)env * A.snap_dw, A.fd, over, comparable);
  if (lane < A.pstride) A.rewards[(size_t)i * A.pstride + lane] = rv;
  if (A.done && lane == 0) A.done[i] = (uint8_t)(over ? 1 : 0);
}

// The snapshot of a consumer that wants REWARDS only (gvec_experience_begin_rewards): the own() planes and the tail of
// SnapLayout, in the same buffer - MAXP * fd + 2 * MAXP + 2 dwords per env (248 bytes at 20x20 4P) instead of the whole
// layout (3.7 KB).  The vis / mask / army sections keep whatever an earlier full snapshot left there: experience records
// need snapshot_kernel.
template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void snapshot_rewards_kernel(ExperienceArgs A) {
  using B = Board<MAXP, NSLOT>;
  const int lane = lane_id();
  const int i = wave_item();
  if (i >= A.num_envs) return;
  const int env = A.env_begin + i;
  B b;
  load_board(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd);
  const SnapLayout<MAXP, NSLOT> L{A.fd};
  uint32_t* sn = A.snap + (size_t)env * A.snap_dw;
  uint32_t tail = 0u;  // as snapshot_kernel: lane p territory, MAXP+p armies, 2*MAXP turn, +1 W|H<<8
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    if (lane < A.fd) sn[L.own() + p * A.fd + lane] = b.own[p];
    const int32_t terr = b.count(b.own[p]), arm = b.army_sum(b.own[p]);
    tail = (lane == p) ? (uint32_t)terr : tail;
    tail = (lane == MAXP + p) ? (uint32_t)arm : tail;
  }
  tail = (lane == 2 * MAXP) ? (uint32_t)b.turn : tail;
  tail = (lane == 2 * MAXP + 1) ? ((uint32_t)b.W | ((uint32_t)b.H << 8)) : tail;
  if (lane < 2 * MAXP + 2) sn[L.tail() + lane] = tail;
}

// CalculateRewardWithConfig (rewards.go:45-85) with the caller's weights (RewardArgs::cfg: kernel arguments, wave-uniform
// scalar loads), for the players of A.players; player p's column is its rank among them.  The same float32 sequence as
// compute_rewards above - with gvec_reward_config_default the two agree bit for bit - then NormalizeReward (:215-223) when
// asked for, the "no predecessor" zero, and invalid_action on top.  Lane k ends with column k's reward, lane 8k + j with term j
// of column k (K <= 8: one dword per lane), so rewards and terms leave as one coalesced store each.
template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void rewards_config_kernel(RewardArgs A) {
  using B = Board<MAXP, NSLOT>;
  const int lane = lane_id();
  const int i = wave_item();
  if (i >= A.num_envs) return;
  B b;
  load_board(b, A.hdr + (size_t)i * HDR_DW, A.rows + (size_t)i * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, i), A.fd);
  const int fd = A.fd;
  const SnapLayout<MAXP, NSLOT> L{fd};
  const uint32_t* sn = A.snap + (size_t)i * A.snap_dw;
  const uint32_t tail = (lane < 2 * MAXP + 2) ? sn[L.tail() + lane] : 0u;
  const int prev_turn = (int)rdlane(tail, 2 * MAXP);
  const uint32_t prev_dims = rdlane(tail, 2 * MAXP + 1);
  const bool comparable = prev_dims == ((uint32_t)b.W | ((uint32_t)b.H << 8)) && b.turn > prev_turn;   // compute_rewards' rule
  const int na = __builtin_popcount(b.alive);
  const bool over = na <= 1;                                               // GameState.IsGameOver (state.go:73-82)
  const int winner = (na == 1) ? (31 - __builtin_clz(b.alive)) : -1;       // GameState.GetWinner (state.go:85-100)
  uint32_t prev_own[MAXP], prev_any = 0u;
  int32_t cur_arm[MAXP], total = 0;
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    prev_own[p] = (lane < fd) ? sn[L.own() + p * fd + lane] : 0u;
    prev_any |= prev_own[p];
    cur_arm[p] = b.army_sum(b.own[p]);
    total += cur_arm[p];
  }
  const gvec_reward_config& c = A.cfg;
  const bool clip = (c.flags & GVEC_REWARD_CLIP) != 0u;
  const int j = lane & 7;
  float rv = 0.0f;
  int32_t tv = 0;
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    if (((A.players >> p) & 1u) == 0u) continue;                            // wave-uniform
    const int col = __builtin_popcount(A.players & ((1u << p) - 1u));
    const int d_terr = b.count(b.own[p]) - (int)rdlane(tail, p);            // :59-62
    const int d_arm = cur_arm[p] - (int)rdlane(tail, MAXP + p);             // :65-68
    const int c_gain = b.count(b.city & b.own[p] & ~prev_own[p]);           // countCityChanges :110-129
    const int c_lost = b.count(b.city & prev_own[p] & ~b.own[p]);
    const int g_gain = b.count(b.gen & b.own[p] & ~prev_own[p] & prev_any); // countGeneralChanges :132-151
    const int g_lost = b.count(b.gen & prev_own[p] & ~b.own[p]);
    const int pa = cur_arm[p], ea = total - cur_arm[p];                     // calculateArmyAdvantage :153-175
    const float adv = (total == 0) ? 0.0f : ((float)(pa - ea) / (float)total);
    float r = 0.0f;
    r += (float)d_terr * c.territory;
    r += (float)d_arm * c.army;
    r += (float)c_gain * c.capture_city;
    r += (float)c_lost * c.lose_city;
    r += (float)g_gain * c.capture_general;
    r += (float)g_lost * c.lose_general;
    r += adv * c.army_advantage;
    int outcome = 0;
    if (over && winner == p) {                                              // :49-56
      r = c.win_game;
      outcome = 1;
    } else if (over && winner != -1) {
      r = c.lose_game;
      outcome = -1;
    }
    if (clip) r = (r > 1.0f) ? 1.0f : ((r < -1.0f) ? -1.0f : r);            // NormalizeReward :215-223
    const bool live = comparable && p < b.P;
    rv = (lane == col) ? (live ? r : 0.0f) : rv;
    int32_t t = d_terr;
    t = (j == 1) ? d_arm : t;
    t = (j == 2) ? c_gain : t;
    t = (j == 3) ? c_lost : t;
    t = (j == 4) ? g_gain : t;
    t = (j == 5) ? g_lost : t;
    t = (j == 6) ? outcome : t;
    t = (j == 7) ? (int32_t)__float_as_uint(adv) : t;
    tv = ((lane >> 3) == col) ? (live ? t : 0) : tv;
  }
  if (lane < A.nk) {
    const size_t at = (size_t)i * A.nk + lane;
    if (A.invalid && A.invalid[at] != 0) rv = rv + c.invalid_action;
    if (A.rewards) A.rewards[at] = rv;
  }
  if (A.terms && lane < 8 * A.nk) A.terms[(size_t)i * 8 * A.nk + lane] = tv;
  if (A.done && lane == 0) A.done[i] = (uint8_t)(over ? 1 : 0);
}

// One EXPERIENCE RECORD per env transition: everything SimpleCollector.OnStateTransition (internal/experience/
// collector.go:30-98) puts into the experiencepb.Experience of every player that acted, in compact form -
// bit-planes and u16 armies instead of 2 x P x [9][H][W] float tensors (3.7 KB instead of 115 KB at 20x20 4P): what a
// rank ships over xGMI to the process that feeds StreamAggregator, which expands it (experience.decode_records).
//   dword 0 currState.Turn | 1 W | H<<8 | P<<16 | flags<<24 (1 done = currState.IsGameOver, 2 fog of war, 4 valid: the env
//   was not re-dealt) | 2 acted bits (players that submitted an action, collector.go:33-37) | 3 env id
//   4.. action index per player (Serializer.ActionToIndex, serializer.go:179-198; -1: none) | rewards f32 per player
//   planes [fd]: prev own[MAXP], prev vis[MAXP], next own[MAXP], next vis[MAXP], general, city, mountain
//   GenerateActionMask(prev) [MAXP][4][fd] | prev armies u16 [NSLOT*64] | next armies u16 [NSLOT*64]
template <int MAXP, int NSLOT>
struct RecordLayout {
  int fd;
  __host__ __device__ int action() const { return 4; }
  __host__ __device__ int reward() const { return 4 + MAXP; }
  __host__ __device__ int planes() const { return 4 + 2 * MAXP; }
  __host__ __device__ int mask() const { return planes() + (4 * MAXP + 3) * fd; }
  __host__ __device__ int army_prev() const { return mask() + 4 * MAXP * fd; }
  __host__ __device__ int army_next() const { return army_prev() + NSLOT * 32; }
  __host__ __device__ int total() const { return (army_next() + NSLOT * 32 + 3) / 4 * 4; }
};

template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void experience_record_kernel(ExperienceArgs A) {
  using B = Board<MAXP, NSLOT>;
  const int lane = lane_id();
  const int i = wave_item();
  if (i >= A.num_envs) return;
  const int env = A.env_begin + i;
  B b;
  load_board(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd);
  const uint32_t* sn = A.snap + (size_t)env * A.snap_dw;
  const SnapLayout<MAXP, NSLOT> S{A.fd};
  const RecordLayout<MAXP, NSLOT> R{A.fd};
  uint32_t* rec = A.records + (size_t)i * A.record_dw;
  bool over, comparable;
  const float rv = compute_rewards<MAXP, NSLOT>(b, sn, A.fd, over, comparable);
  // lane p: player p's action -> Serializer.ActionToIndex(action, prevState.Board.W)
  uint32_t alo = 0u, ahi = 0u;
  if (lane < A.pstride) {
    const uint2 w = reinterpret_cast<const uint2*>(A.actions)[(size_t)env * A.pstride + lane];
    alo = w.x;
    ahi = w.y;
  }
  const int prev_w = (int)(rdlane((lane < 2 * MAXP + 2) ? sn[S.tail() + lane] : 0u, 2 * MAXP + 1) & 0xFFu);
  const int fx = (int)(int8_t)(alo & 0xFFu), fy = (int)(int8_t)((alo >> 8) & 0xFFu);
  const int dx = (int)(int8_t)((alo >> 16) & 0xFFu) - fx, dy = (int)(int8_t)(alo >> 24) - fy;
  int dir = 0;                                   // :183-195: up 0 (and anything that is not a unit step), down 1, left 2, right 3
  dir = (dx == 0 && dy == 1) ? 1 : dir;
  dir = (dx == -1 && dy == 0) ? 2 : dir;
  dir = (dx == 1 && dy == 0) ? 3 : dir;
  const bool acted = lane < b.P && (ahi & GVEC_ACT_VALID) != 0u;
  const int aidx = acted ? ((fy * prev_w + fx) * 4 + dir) : -1;
  const uint32_t acted_bits = (uint32_t)__builtin_amdgcn_ballot_w64(acted);
  if (lane < MAXP) {
    rec[R.action() + lane] = (uint32_t)aidx;
    rec[R.reward() + lane] = __float_as_uint(rv);
  }
  if (lane == 0) {
    rec[0] = (uint32_t)b.turn;
    rec[1] = (uint32_t)b.W | ((uint32_t)b.H << 8) | ((uint32_t)b.P << 16) |
             (((over ? 1u : 0u) | ((b.hflags & HF_FOG) ? 2u : 0u) | (comparable ? 4u : 0u)) << 24);
    rec[2] = acted_bits;
    rec[3] = (uint32_t)(A.env_id_base + env);
  }
  if (lane < A.fd) {
    uint32_t* pl = rec + R.planes() + lane;
#pragma unroll
    for (int p = 0; p < MAXP; ++p) {
      pl[p * A.fd] = sn[S.own() + p * A.fd + lane];
      pl[(MAXP + p) * A.fd] = sn[S.vis() + p * A.fd + lane];
      pl[(2 * MAXP + p) * A.fd] = b.own[p];
      pl[(3 * MAXP + p) * A.fd] = b.vis[p];
    }
    pl[(4 * MAXP + 0) * A.fd] = b.gen;
    pl[(4 * MAXP + 1) * A.fd] = b.city;
    pl[(4 * MAXP + 2) * A.fd] = b.mtn;
  }
  for (int k = lane; k < 4 * MAXP * A.fd; k += 64) rec[R.mask() + k] = sn[S.mask() + k];
  for (int k = lane; k < NSLOT * 32; k += 64) rec[R.army_prev() + k] = sn[S.army() + k];
  store_army_sat16<NSLOT>(b.army, rec + R.army_next());
  for (int k = R.army_next() + NSLOT * 32 + lane; k < A.record_dw; k += 64) rec[k] = 0u;
}

// The consumer side of the exchange step: expands compact experience records - on whatever GPU they were
// gathered to - into what SimpleCollector.OnStateTransition (collector.go:41-75) puts into every acting player's
// experiencepb.Experience: StateToTensor(prevState, p), StateToTensor(currState, p) ([9][H][W] float32, serializer.go:37-109),
// GenerateActionMask(prevState, p) ([]bool, index t*4 + d, d = 0 up, 1 down, 2 left, 3 right, :112-176), and the scalar
// fields.  One wavefront per record; needs no engine handle (the record carries its own W, H, P, flags; the layout
// constants arrive as arguments).  A u16 army saturated at 65,535 is exact here: the tensor clamps army / 1000 at 1.
struct ExpandArgs {
  const uint32_t* records;  // [n][record_dw]
  float* state;             // [n][mp][9*stride]
  float* next_state;        // [n][mp][9*stride]
  uint8_t* mask;            // [n][mp][4*stride] 0/1 bytes
  int32_t* meta;            // [n][mp][8]: present (valid record & the player acted), env id, player, turn, action, reward bits, done, W | H << 8
  int32_t n, record_dw, mp, fd, ns, stride;
};

// own / vis / types / army: this wave's LDS copy of the record; any: OR of the P ownership planes
// One StateToTensor of an expanded record.  Its nine planes are N = W*H floats each, back to back: for most boards no plane
// starts on a 256-byte boundary (15x15: 900 bytes; 20x20: 1,600), and stores of "tiles 64j .. 64j+63" that begin anywhere
// in a line leave at a third of the rate of aligned ones (32,768 records: 15x15 and 25x25 expanded at 1.9 TB/s, 16x16 and
// 32x32 at 5.9-6.3).  So every store covers an ALIGNED window of 64 floats: lane l of window k holds tile 64k - sh + l of its
// plane (sh: the plane's dword offset inside its 256-byte line); the bits come from the record in LDS, where any tile is
// as near as any other.
__device__ __forceinline__ void expand_tensor(float* out, const uint32_t* own_p, const uint32_t* any, const uint32_t* vis_p, const uint32_t* types,
                                              const uint16_t* army, int fd, int N, int stride, bool fog) {
  const int lane = lane_id();
  const uint32_t a0 = (uint32_t)(reinterpret_cast<uintptr_t>(out) >> 2);
  if (((a0 | (uint32_t)N) & 3u) == 0u) {
    // planes of a multiple of four floats on 16-byte boundaries (10x10, 16x16, 20x20, 32x32 ...): FOUR neighbouring tiles per
    // lane - a nibble of each of the record's planes, four u16 armies in one LDS read, nine 1-KB stores per 256 tiles, which
    // (unlike 256-byte runs of dwords) leave at full rate wherever they start
    auto nib = [&](const uint32_t* plane, int q) { return (plane[q >> 3] >> ((q & 7) << 2)) & 15u; };
    for (int q = lane; q < (N >> 2); q += 64) {
      const uint32_t n_any = nib(any, q), n_mine = nib(own_p, q), n_seen = nib(vis_p, q);
      const uint32_t n_spec = nib(types, q) | nib(types + fd, q), n_mtn = nib(types + 2 * fd, q);
      const uint32_t n_vis = fog ? n_seen : 15u;                   // :50
      const uint32_t n_open = n_vis & ~n_mtn;                      // mountains short-circuit (:68-71)
      const uint32_t* ap = reinterpret_cast<const uint32_t*>(army) + 2 * q;    // the record's armies are dword-aligned in LDS
      const uint2 aw = make_uint2(ap[0], ap[1]);
      auto arm = [](uint32_t a) {
        float norm = (float)(int)a / 1000.0f;                      // :82-85
        norm = norm > 1.0f ? 1.0f : norm;
        return (a > 0u) ? norm : 0.0f;
      };
      const float r0 = arm(aw.x & 0xFFFFu), r1 = arm(aw.x >> 16), r2 = arm(aw.y & 0xFFFFu), r3 = arm(aw.y >> 16);
      const size_t n = (size_t)N;
      auto put = [&](int c, uint32_t m, float v0, float v1, float v2, float v3) {
        float4 o;
        o.x = (m & 1u) ? v0 : 0.0f;
        o.y = (m & 2u) ? v1 : 0.0f;
        o.z = (m & 4u) ? v2 : 0.0f;
        o.w = (m & 8u) ? v3 : 0.0f;
        st_stream<GVEC_NT_MASK>(reinterpret_cast<u32x4*>(out + c * n) + q, *reinterpret_cast<const u32x4*>(&o));
      };
      const uint32_t m_mine = n_open & n_mine, m_other = n_open & ~n_mine & n_any;
      put(0, m_mine, r0, r1, r2, r3);
      put(1, m_other, r0, r1, r2, r3);
      put(2, m_mine, 1.0f, 1.0f, 1.0f, 1.0f);
      put(3, m_other, 1.0f, 1.0f, 1.0f, 1.0f);
      put(4, n_open & ~n_any, 1.0f, 1.0f, 1.0f, 1.0f);
      put(5, n_open & n_spec, 1.0f, 1.0f, 1.0f, 1.0f);
      put(6, n_vis & n_mtn, 1.0f, 1.0f, 1.0f, 1.0f);
      put(7, n_vis, 1.0f, 1.0f, 1.0f, 1.0f);
      put(8, ~n_vis & 15u, 1.0f, 1.0f, 1.0f, 1.0f);
    }
  } else
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    float* plane = out + (size_t)c * (size_t)N;
    const int sh = (int)((a0 + (uint32_t)c * (uint32_t)N) & 63u);
    for (int t = lane - sh; t < N; t += 64) {
      if (t < 0) continue;
      const int dwi = t >> 5;
      const uint32_t bit = 1u << (t & 31);
      const bool seen = (vis_p[dwi] & bit) != 0u, mount = (types[2 * fd + dwi] & bit) != 0u;
      const bool visible = !fog || seen;      // :50
      const bool open = visible && !mount;    // mountains short-circuit (:68-71)
      float v;
      if (c <= 3) {
        const bool owned = (any[dwi] & bit) != 0u, mine = (own_p[dwi] & bit) != 0u;
        const bool who = (c & 1) ? (!mine && owned) : mine;      // 0, 2: the player's own; 1, 3: somebody else's
        if (c < 2) {
          const int a = (int)army[t];
          float norm = (float)a / 1000.0f;    // :82-85
          norm = norm > 1.0f ? 1.0f : norm;
          v = (open && who && a > 0) ? norm : 0.0f;
        } else {
          v = (open && who) ? 1.0f : 0.0f;
        }
      } else if (c == 4) {
        v = (open && !(any[dwi] & bit)) ? 1.0f : 0.0f;
      } else if (c == 5) {
        v = (open && ((types[dwi] | types[fd + dwi]) & bit)) ? 1.0f : 0.0f;
      } else if (c == 6) {
        v = (visible && mount) ? 1.0f : 0.0f;
      } else {
        v = (visible == (c == 7)) ? 1.0f : 0.0f;
      }
      st_stream<GVEC_NT_MASK>(plane + t, v);
    }
  }
  for (int i = 9 * N + lane; i < 9 * stride; i += 64) out[i] = 0.0f;  // a smaller board in a padded batch: clear the rest of the slot
}

// dynamic LDS: per wave the record (record_dw dwords) + two fd-dword "anybody owns it" planes (prev, next)
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void expand_records_kernel(ExpandArgs A) {
  extern __shared__ uint32_t expand_lds[];
  const int wave = block_wave(), lane = lane_id();
  const int i = wave_item();
  if (i >= A.n) return;
  const int mp = A.mp, fd = A.fd;
  uint32_t* rec = expand_lds + (size_t)wave * (A.record_dw + 2 * fd);
  {
    const uint32_t* g = A.records + (size_t)i * A.record_dw;
    for (int k = lane; k < A.record_dw; k += 64) rec[k] = g[k];
  }
  wave_lds_fence();
  const uint32_t r1 = rec[1];
  int W = (int)(r1 & 0xFFu), H = (int)((r1 >> 8) & 0xFFu), P = (int)((r1 >> 16) & 0xFFu);
  const uint32_t flags = r1 >> 24;
  const bool ok = W >= 1 && H >= 1 && W * H <= A.stride && P >= 1 && P <= mp;   // a malformed record expands to nothing
  if (!ok) W = H = P = 0;
  const int N = W * H;
  const uint32_t acted = ok && (flags & 4u) ? rec[2] : 0u;   // a void record (re-dealt env) yields no experience
  const int off_planes = 4 + 2 * mp, off_mask = off_planes + (4 * mp + 3) * fd, off_prev = off_mask + 4 * mp * fd, off_next = off_prev + A.ns * 32;
  const uint32_t* prev_own = rec + off_planes;
  const uint32_t* prev_vis = prev_own + mp * fd;
  const uint32_t* next_own = prev_vis + mp * fd;
  const uint32_t* next_vis = next_own + mp * fd;
  const uint32_t* types = next_vis + mp * fd;   // general, city, mountain
  const uint16_t* army_prev = reinterpret_cast<const uint16_t*>(rec + off_prev);
  const uint16_t* army_next = reinterpret_cast<const uint16_t*>(rec + off_next);
  uint32_t* any_prev = rec + A.record_dw;
  uint32_t* any_next = any_prev + fd;
  if (lane < fd) {
    uint32_t a = 0u, b = 0u;
    for (int q = 0; q < P; ++q) {
      a |= prev_own[q * fd + lane];
      b |= next_own[q * fd + lane];
    }
    any_prev[lane] = a;
    any_next[lane] = b;
  }
  wave_lds_fence();
  for (int p = 0; p < mp; ++p) {
    const size_t slot = (size_t)i * mp + p;
    const bool present = p < P && ((acted >> p) & 1u) != 0u;
    int32_t* meta = A.meta + slot * 8;
    if (lane < 8) {
      int32_t v = 0;
      v = (lane == 0) ? (present ? 1 : 0) : v;
      v = (lane == 1) ? (int32_t)rec[3] : v;
      v = (lane == 2) ? p : v;
      v = (lane == 3) ? (int32_t)rec[0] : v;
      v = (lane == 4) ? (int32_t)rec[4 + p] : v;
      v = (lane == 5) ? (int32_t)rec[4 + mp + p] : v;
      v = (lane == 6) ? (int32_t)(flags & 1u) : v;
      v = (lane == 7) ? (int32_t)((uint32_t)W | ((uint32_t)H << 8)) : v;
      meta[lane] = present ? v : ((lane == 2) ? p : 0);
    }
    float* st = A.state + slot * 9 * (size_t)A.stride;
    float* nx = A.next_state + slot * 9 * (size_t)A.stride;
    uint8_t* mk = A.mask + slot * 4 * (size_t)A.stride;
    if (!present) {  // wave-uniform
      for (int k = lane; k < 9 * A.stride; k += 64) st[k] = nx[k] = 0.0f;
      for (int k = lane; k < A.stride; k += 64) reinterpret_cast<uint32_t*>(mk)[k] = 0u;
      continue;
    }
    expand_tensor(st, prev_own + p * fd, any_prev, prev_vis + p * fd, types, army_prev, fd, N, A.stride, (flags & 2u) != 0u);
    expand_tensor(nx, next_own + p * fd, any_next, next_vis + p * fd, types, army_next, fd, N, A.stride, (flags & 2u) != 0u);
    // GenerateActionMask as bytes, four per tile (t*4 + d): one dword store per tile
    const uint32_t* m = rec + off_mask + p * 4 * fd;   // [d][fd]
    const int msh = (int)((reinterpret_cast<uintptr_t>(mk) >> 2) & 63u);       // aligned windows here too
    for (int t = lane - msh; t < A.stride; t += 64) {
      if (t < 0) continue;
      uint32_t v = 0u;
      if (t < N) {
        const int dwi = t >> 5, sh = t & 31;
        v = ((m[dwi] >> sh) & 1u) | (((m[fd + dwi] >> sh) & 1u) << 8) | (((m[2 * fd + dwi] >> sh) & 1u) << 16) | (((m[3 * fd + dwi] >> sh) & 1u) << 24);
      }
      st_stream<GVEC_NT_MASK>(reinterpret_cast<uint32_t*>(mk) + t, v);
    }
  }
}

// Serializer.StateToTensor (internal/experience/serializer.go:37-109): [9][H][W] float32 from one
// player's perspective; the output is 9 coalesced channel planes per 64-tile slot.
template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void observe_kernel(ExperienceArgs A) {
  using B = Board<MAXP, NSLOT>;
  const int lane = lane_id();
  const int env = wave_item();
  if (env >= A.num_envs) return;
  B b;
  load_board(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd);
  const bool fog_on = (b.hflags & HF_FOG) != 0u;
  uint32_t own_any = 0u;
#pragma unroll
  for (int p = 0; p < MAXP; ++p) own_any |= b.own[p];
  const uint32_t special = b.gen | b.city;
  const int p_lo = (A.player < 0) ? 0 : A.player, p_hi = (A.player < 0) ? A.pstride : A.player + 1;
  for (int pl = p_lo; pl < p_hi; ++pl) {
    float* out = A.obs + ((A.player < 0) ? ((size_t)env * A.pstride + pl) : (size_t)env) * 9 * (size_t)A.stride;
    uint32_t own_p = 0u, vis_p = 0u;
#pragma unroll
    for (int p = 0; p < MAXP; ++p) {
      own_p = (p == pl) ? b.own[p] : own_p;
      vis_p = (p == pl) ? b.vis[p] : vis_p;
    }
    const uint32_t a0 = (uint32_t)(reinterpret_cast<uintptr_t>(out) >> 2);
    if (((a0 | (uint32_t)b.N) & 63u) != 0u) {
      // planes that do not start on 256-byte boundaries (all boards but 16x16, 32x32 ...): aligned 64-float store windows, as
      // in gym_emit below.  65,536 envs, one player: 15x15 0.297 -> 0.157 ms, 25x25 0.790 -> 0.365, 10x10 0.110 -> 0.079,
      // 20x20 0.200 -> 0.170 (5.6 TB/s)
      // (every at() / army_at() is a ds_bpermute: evaluated by all lanes, never behind a lane-dependent `&&`)
      auto at = [&](uint32_t plane, int t) { return __builtin_amdgcn_ubfe(bperm((t >> 5) << 2, plane), (uint32_t)(t & 31), 1u) != 0u; };
      auto emit = [&](int c, auto&& value) {
        float* base = out + (size_t)c * (size_t)b.N;
        const int sh = (int)((a0 + (uint32_t)c * (uint32_t)b.N) & 63u);
#pragma unroll
        for (int k = 0; k <= NSLOT; ++k) {
          if (64 * k - sh < b.N) {                   // wave-uniform
            const int t = 64 * k - sh + lane;
            const bool ok = t >= 0 && t < b.N;
            const int tt = ok ? t : 0;
            const bool seen = at(vis_p, tt), mount = at(b.mtn, tt);
            const bool visible = !fog_on || seen;    // :50
            const float v = value(k, tt, sh, visible, visible && !mount, mount);   // open: mountains short-circuit (:68-71)
            if (ok) st_stream<GVEC_NT_MASK>(base + t, v);
          }
        }
      };
      auto arm_at = [&](int k, int sh) {             // tile 64k - sh + l: slot k (lanes l >= sh) or k - 1, sh lanes further on
        const int from = ((lane - sh) & 63) << 2;
        const int32_t cur = (int32_t)bperm(from, (uint32_t)b.army[k < NSLOT ? k : NSLOT - 1]);
        const int32_t prv = (int32_t)bperm(from, (uint32_t)b.army[k > 0 ? k - 1 : 0]);
        const int32_t a = (lane >= sh) ? cur : prv;
        float norm = (float)a / 1000.0f;             // :82-85
        norm = norm > 1.0f ? 1.0f : norm;
        return (a > 0) ? norm : 0.0f;
      };
      emit(0, [&](int k, int t, int sh, bool, bool open, bool) { const bool mine = at(own_p, t); const float arm = arm_at(k, sh); return (open && mine) ? arm : 0.0f; });
      emit(1, [&](int k, int t, int sh, bool, bool open, bool) {
        const bool mine = at(own_p, t), owned = at(own_any, t);
        const float arm = arm_at(k, sh);
        return (open && !mine && owned) ? arm : 0.0f;
      });
      emit(2, [&](int, int t, int, bool, bool open, bool) { const bool mine = at(own_p, t); return (open && mine) ? 1.0f : 0.0f; });
      emit(3, [&](int, int t, int, bool, bool open, bool) { const bool mine = at(own_p, t), owned = at(own_any, t); return (open && !mine && owned) ? 1.0f : 0.0f; });
      emit(4, [&](int, int t, int, bool, bool open, bool) { const bool owned = at(own_any, t); return (open && !owned) ? 1.0f : 0.0f; });
      emit(5, [&](int, int t, int, bool, bool open, bool) { const bool spec = at(special, t); return (open && spec) ? 1.0f : 0.0f; });
      emit(6, [&](int, int, int, bool visible, bool, bool mount) { return (visible && mount) ? 1.0f : 0.0f; });
      emit(7, [&](int, int, int, bool visible, bool, bool) { return visible ? 1.0f : 0.0f; });
      emit(8, [&](int, int, int, bool visible, bool, bool) { return visible ? 0.0f : 1.0f; });
    } else
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const int t = 64 * s + lane;
      const bool mine = gather(own_p, s) != 0u, owned = gather(own_any, s) != 0u, seen = gather(vis_p, s) != 0u;
      const bool spec = gather(special, s) != 0u, mount = gather(b.mtn, s) != 0u;
      const bool visible = !fog_on || seen;  // :50
      const bool open = visible && !mount;   // mountains short-circuit (:68-71)
      float norm = (float)b.army[s] / 1000.0f;  // :82-85
      norm = norm > 1.0f ? 1.0f : norm;
      const float arm = (b.army[s] > 0) ? norm : 0.0f;
      if (t < b.N) {
        const size_t n = (size_t)b.N;
        // 14.4 KB per (env, player) that the kernel never reads back: streamed past the L2 like the turn's own stores
        st_stream<GVEC_NT_MASK>(out + 0 * n + t, (open && mine) ? arm : 0.0f);
        st_stream<GVEC_NT_MASK>(out + 1 * n + t, (open && !mine && owned) ? arm : 0.0f);
        st_stream<GVEC_NT_MASK>(out + 2 * n + t, (open && mine) ? 1.0f : 0.0f);
        st_stream<GVEC_NT_MASK>(out + 3 * n + t, (open && !mine && owned) ? 1.0f : 0.0f);
        st_stream<GVEC_NT_MASK>(out + 4 * n + t, (open && !owned) ? 1.0f : 0.0f);
        st_stream<GVEC_NT_MASK>(out + 5 * n + t, (open && spec) ? 1.0f : 0.0f);
        st_stream<GVEC_NT_MASK>(out + 6 * n + t, (visible && mount) ? 1.0f : 0.0f);
        st_stream<GVEC_NT_MASK>(out + 7 * n + t, visible ? 1.0f : 0.0f);
        st_stream<GVEC_NT_MASK>(out + 8 * n + t, visible ? 0.0f : 1.0f);
      }
    }
    // a smaller board in a padded batch: clear the rest of the slot
    for (int i = 9 * b.N + lane; i < 9 * A.stride; i += 64) out[i] = 0.0f;
  }
}

// =========================================================================================
// host-side launchers
// =========================================================================================
hipError_t launch_snapshot(const Variant& v, const ExperienceArgs& a, hipStream_t s) {
  return dispatch(v, [&](auto P, auto S) { return launch_waves(snapshot_kernel<P, S>, a.num_envs, s, a); });
}
hipError_t launch_rewards(const Variant& v, const ExperienceArgs& a, hipStream_t s) {
  return dispatch(v, [&](auto P, auto S) { return launch_waves(rewards_kernel<P, S>, a.num_envs, s, a); });
}
hipError_t launch_snapshot_rewards(const Variant& v, const ExperienceArgs& a, hipStream_t s) {
  return dispatch(v, [&](auto P, auto S) { return launch_waves(snapshot_rewards_kernel<P, S>, a.num_envs, s, a); });
}
hipError_t launch_rewards_config(const Variant& v, const RewardArgs& a, hipStream_t s) {
  return dispatch(v, [&](auto P, auto S) { return launch_waves(rewards_config_kernel<P, S>, a.num_envs, s, a); });
}
hipError_t launch_experience_records(const Variant& v, const ExperienceArgs& a, hipStream_t s) {
  return dispatch(v, [&](auto P, auto S) { return launch_waves(experience_record_kernel<P, S>, a.num_envs, s, a); });
}
hipError_t launch_observe(const Variant& v, const ExperienceArgs& a, hipStream_t s) {
  return dispatch(v, [&](auto P, auto S) { return launch_waves(observe_kernel<P, S>, a.num_envs, s, a); });
}
void experience_layout(const Variant& v, int fd, int* snap_dw, int* record_dw) {
  (void)dispatch(v, [&](auto P, auto S) {
    *snap_dw = SnapLayout<P, S>{fd}.total();
    *record_dw = RecordLayout<P, S>{fd}.total();
    return hipSuccess;
  });
}
hipError_t launch_expand_records(const void* records, int32_t n, const int32_t* layout8, float* state, float* next_state, uint8_t* mask,
                                 int32_t* meta, hipStream_t s) {
  ExpandArgs a;
  a.records = reinterpret_cast<const uint32_t*>(records);
  a.state = state;
  a.next_state = next_state;
  a.mask = mask;
  a.meta = meta;
  a.n = n;
  a.record_dw = layout8[0];
  a.mp = layout8[1];
  a.fd = layout8[2];
  a.ns = layout8[3];
  a.stride = layout8[5];
  const size_t lds = (size_t)WAVES_PER_BLOCK * (a.record_dw + 2 * a.fd) * 4;   // <= 52 KB (32x32 8P)
  return launch_waves(expand_records_kernel, n, lds, s, a);
}

}  // namespace gvec
