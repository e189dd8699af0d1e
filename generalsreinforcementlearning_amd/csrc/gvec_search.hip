// gvec_search.hip — flat Monte Carlo search (gvec_search_playouts): one wavefront per playout loads a root
// board read-only, plays one candidate action for one seat, then random-agent turns, and writes back eight numbers instead
// of a board.
#include "gvec_dispatch.hpp"
#include "gvec_turn.hpp"

namespace gvec {

// Playout v = (i * K + k) * R + j is root i, candidate k, replica j.  The root is never written: the header (its lifetime
// counters included), the planes, the armies, the legal-mask buffer, err and the recorded actions stay byte for byte.
//   load    root_envs[i] (null: i) and root_players[i], wave-uniform; load_turn as rollout_kernel loads (run-time strides)
//   decode  candidates[i][k] against the seat's gym view of the root, as gym_step_players_kernel decodes a learner's action.
//           GVEC_SEARCH_PASS plays no move for the seat on turn 0.  The row is INVALID - all zeros, nothing is played - for any
//           other action that is not accepted (GVEC_SEARCH_NONE, the padding, among them), a root env out of range, a root
//           that is over, a seat that is not alive (alive implies below the env's player count).
//   turn 0  the agent's draw for every seat under the key of the PLAYOUT (env_key_of(seed_base, v), not the root env's), the
//           seat's lane of the ActVec overwritten with the candidate as gym_play_turn's learner_moves does
//   turns 1 .. depth - 1: rollout_kernel's inner loop.  A finished game ends the playout; it is never re-dealt.
//   terms[v][8]: valid, turns, alive, won, land, army, land_others, army_others - the counts from the sources the gym
//           kernels use (turn_tile_counts, army_counts)
template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, (rollout_waves<MAXP, NSLOT>())) void search_kernel(StepArgs A, SearchArgs S) {
  __shared__ int32_t army_shadow[WAVES_PER_BLOCK][NSLOT * 64];
  using B = Turn<MAXP, NSLOT>;
  __shared__ uint32_t act_scratch[WAVES_PER_BLOCK][B::ACT_SCRATCH_DW];
  const int wave = block_wave(), lane = lane_id();
  const int v = wave_item();
  if (v >= S.num_playouts) return;
  const int per_root = S.num_candidates * S.replicas;
  const int i = v / per_root, k = (v - i * per_root) / S.replicas;
  const int env = S.root_envs ? uni(S.root_envs[i]) : i;
  const int pl = uni(S.root_players[i]);
  const long long a = (long long)uni64((uint64_t)S.candidates[(size_t)i * S.num_candidates + k]);
  int32_t* out = S.terms + (size_t)v * GVEC_SEARCH_TERMS;
  if (env < 0 || env >= A.num_envs) {   // wave-uniform; checked here, so that the call needs no host copy of the ids
    if (lane < GVEC_SEARCH_TERMS) out[lane] = 0;
    return;
  }
  B b;
  b.larmy = army_shadow[wave];
  b.lscr = act_scratch[wave];
  load_turn(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd, A.zeros);
  const bool seat_ok = pl >= 0 && pl < MAXP && ((b.alive >> (pl & 31)) & 1u) != 0u;
  const int seat = seat_ok ? pl : 0;   // the view of a seat the board has: every lane takes part in the cross-lane reads below
  const GymMove mv = gym_decode(b, gym_sources(b, turn_view(b, seat)), a, S.stride);
  const bool pass = a == (long long)GVEC_SEARCH_PASS;
  if (!seat_ok || (b.hflags & HF_DONE) || !(pass || mv.accepted)) {   // wave-uniform
    if (lane < GVEC_SEARCH_TERMS) out[lane] = 0;
    return;
  }
  const uint32_t c_meta = pass ? 0u : (16u | (mv.half ? 32u : 0u));
  uint32_t m[B::NR][4];
  const uint32_t ek = env_key_of(A.seed_base, (uint32_t)v);
  int t = 0;
  b.template legal_planes<false>(m);
  while (t < S.depth && !(b.hflags & HF_DONE)) {
    const uint32_t mine = agent_sample<MAXP, NSLOT>(b, m, ek, A);
    typename B::ActVec av = agent_actvec<MAXP, NSLOT>(b, mine, A.invalid_permille > 0);
    const bool cand = t == 0 && lane == seat;   // turn 0: the seat's slot is the candidate
    av.meta = cand ? c_meta : av.meta;
    av.ft = cand ? mv.from : av.ft;
    av.tt = cand ? mv.tt : av.tt;
    bool aborted;
    (void)b.turn_step(av, A, aborted);
    ++t;
    b.refresh_gt1();
    b.template legal_planes<false>(m);
  }
  const uint32_t tcl = turn_tile_counts(b), acl = army_counts<MAXP>(b);
  const bool other = lane < MAXP && lane != seat;
  const uint32_t land = rdlane(tcl, seat), army = rdlane(acl, seat);
  const uint32_t land_others = wave_sum(other ? tcl : 0u), army_others = wave_sum(other ? acl : 0u);
  const bool over = (b.hflags & HF_DONE) != 0u;
  const uint32_t alive = (b.alive >> seat) & 1u, won = (over && gym_winner(over, b.P, b.alive) == seat) ? 1u : 0u;
  const uint32_t val = lane == 0 ? 1u : lane == 1 ? (uint32_t)t : lane == 2 ? alive : lane == 3 ? won : lane == 4 ? land : lane == 5 ? army
                       : lane == 6 ? land_others : army_others;
  if (lane < GVEC_SEARCH_TERMS) out[lane] = (int32_t)val;
}

hipError_t launch_search(const Variant& v, const StepArgs& in, const SearchArgs& g, hipStream_t s) {
  StepArgs keyed = in;
  keyed.env_base = 0;   // the playout index is the key, whichever handle the roots live in
  const StepArgs a = with_seed_bases(keyed);
  return dispatch(v, [&](auto P, auto S) { return launch_waves(search_kernel<P, S>, g.num_playouts, s, a, g); });
}

}  // namespace gvec
