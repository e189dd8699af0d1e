// gvec_search.hip — flat Monte Carlo search (gvec_search_playouts, gvec_search_playouts_bot): one
// wavefront per playout loads a root board read-only, plays one candidate action for one seat, then random-agent turns - or
// turns in which named seats play the scripted opponent's rule (gvec_bot.hpp) - and writes back eight numbers instead of a
// board.  gvec_search_expand's pair of kernels (gvec_tree.hip) is the same playout that also keeps the board after
// its first turn; what all four share is gvec_search.hpp.
#include "gvec_bot.hpp"
#include "gvec_dispatch.hpp"
#include "gvec_search.hpp"
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
// What the two kernels share is the helpers of gvec_search.hpp; only the turn loop differs.  They take and return plain values: a helper
// that returns the row through references, or one that holds the two early returns, compiles search_kernel to other
// instructions than before (all 18 instantiations), and these do not.

template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, (rollout_waves<MAXP, NSLOT>())) void search_kernel(StepArgs A, SearchArgs S) {
  __shared__ int32_t army_shadow[WAVES_PER_BLOCK][NSLOT * 64];
  using B = Turn<MAXP, NSLOT>;
  __shared__ uint32_t act_scratch[WAVES_PER_BLOCK][B::ACT_SCRATCH_DW];
  const int wave = block_wave(), lane = lane_id();
  const int v = wave_item();
  if (v >= S.num_playouts) return;
  int k;
  const int i = search_root_index(S, v, k);
  const int env = search_root_env(S, i);
  const int pl = uni(S.root_players[i]);
  const long long a = search_candidate(S, i, k);
  int32_t* out = S.terms + (size_t)v * GVEC_SEARCH_TERMS;
  if (env < 0 || env >= A.num_envs) {   // wave-uniform; checked here, so that the call needs no host copy of the ids
    search_invalid_row(out, lane);
    return;
  }
  B b;
  b.larmy = army_shadow[wave];
  b.lscr = act_scratch[wave];
  load_turn(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd, A.zeros);
  const bool seat_ok = search_seat_ok<MAXP>(b.alive, pl);
  const int seat = seat_ok ? pl : 0;   // the view of a seat the board has: every lane takes part in the cross-lane reads below
  const GymMove mv = gym_decode(b, gym_sources(b, turn_view(b, seat)), a, S.stride);
  const bool pass = a == (long long)GVEC_SEARCH_PASS;
  if (!seat_ok || (b.hflags & HF_DONE) || !(pass || mv.accepted)) {   // wave-uniform
    search_invalid_row(out, lane);
    return;
  }
  const uint32_t c_meta = search_meta(pass, mv.half);
  uint32_t m[B::NR][4];
  const uint32_t ek = env_key_of(A.seed_base, (uint32_t)v);
  int t = 0;
  b.template legal_planes<false>(m);
  while (t < S.depth && !(b.hflags & HF_DONE)) {
    const uint32_t mine = agent_sample<MAXP, NSLOT>(b, m, ek, A);
    typename B::ActVec av = agent_actvec<MAXP, NSLOT>(b, mine, A.invalid_permille > 0);
    search_override(av, t == 0 && lane == seat, c_meta, mv.from, mv.tt);
    bool aborted;
    (void)b.turn_step(av, A, aborted);
    ++t;
    b.refresh_gt1();
    b.template legal_planes<false>(m);
  }
  search_terms<MAXP, NSLOT>(b, out, seat, lane, t);
}

// The same playout with the seats of G.players on the scripted opponent's rule (gvec_search_playouts_bot):
// every turn is gvec_agent_actions, then gvec_bot_actions(G.players, seed, G.random_permille) over it, then gvec_step, of
// the playout's own board - env v of a scratch handle of n * K * R copies draws what playout v draws, for the agent and for
// the exploration mix alike (both keyed by ek and the board's own turn counter).  Load, decode, invalid rows and terms are
// search_kernel's; a second kernel, not a flag, so that search_kernel's instruction stream stays what it was.
//   The agent's draw comes before bot_sample, which overwrites m; the turn's legal_planes refill it.
//   Every seat the rule can move being a mover (all the living on the rule, no exploration), nobody plays the agent's draw:
//   a seat that is not alive draws no action (agent_sample: act needs alive), so the draw is skipped - wave-uniform.
//   A seat on the rule that finds no move plays none (word 0), as gvec_bot_actions writes it.
template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, (rollout_waves<MAXP, NSLOT>())) void search_bot_kernel(StepArgs A, SearchArgs S, BotArgs G) {
  __shared__ int32_t army_shadow[WAVES_PER_BLOCK][NSLOT * 64];
  using B = Turn<MAXP, NSLOT>;
  __shared__ uint32_t act_scratch[WAVES_PER_BLOCK][B::ACT_SCRATCH_DW];
  const int wave = block_wave(), lane = lane_id();
  const int v = wave_item();
  if (v >= S.num_playouts) return;
  int k;
  const int i = search_root_index(S, v, k);
  const int env = search_root_env(S, i);
  const int pl = uni(S.root_players[i]);
  const long long a = search_candidate(S, i, k);
  int32_t* out = S.terms + (size_t)v * GVEC_SEARCH_TERMS;
  if (env < 0 || env >= A.num_envs) {   // wave-uniform; checked here, so that the call needs no host copy of the ids
    search_invalid_row(out, lane);
    return;
  }
  B b;
  b.larmy = army_shadow[wave];
  b.lscr = act_scratch[wave];
  load_turn(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd, A.zeros);
  const bool seat_ok = search_seat_ok<MAXP>(b.alive, pl);
  const int seat = seat_ok ? pl : 0;   // the view of a seat the board has: every lane takes part in the cross-lane reads below
  const GymMove mv = gym_decode(b, gym_sources(b, turn_view(b, seat)), a, S.stride);
  const bool pass = a == (long long)GVEC_SEARCH_PASS;
  if (!seat_ok || (b.hflags & HF_DONE) || !(pass || mv.accepted)) {   // wave-uniform
    search_invalid_row(out, lane);
    return;
  }
  const uint32_t c_meta = search_meta(pass, mv.half);
  uint32_t m[B::NR][4];
  const uint32_t ek = env_key_of(A.seed_base, (uint32_t)v);
  int t = 0;
  b.template legal_planes<false>(m);
  while (t < S.depth && !(b.hflags & HF_DONE)) {
    const uint32_t rnd_bits = G.random_permille > 0 ? bot_random_seats<MAXP>(ek, (uint32_t)b.turn, G.random_permille) : 0u;
    const uint32_t movers = G.players & b.alive & ~rnd_bits;
    uint32_t agent_mine = 0u;
    if (movers != b.alive) agent_mine = agent_sample<MAXP, NSLOT>(b, m, ek, A);   // somebody alive plays the agent's draw
    const uint32_t bot_mine = bot_sample<MAXP, NSLOT>(b, m, movers);
    const uint32_t mine = ((movers >> lane) & 1u) ? bot_mine : agent_mine;
    typename B::ActVec av = agent_actvec<MAXP, NSLOT>(b, mine, A.invalid_permille > 0);
    search_override(av, t == 0 && lane == seat, c_meta, mv.from, mv.tt);
    bool aborted;
    (void)b.turn_step(av, A, aborted);
    ++t;
    b.refresh_gt1();
    b.template legal_planes<false>(m);
  }
  search_terms<MAXP, NSLOT>(b, out, seat, lane, t);
}

hipError_t launch_search(const Variant& v, const StepArgs& in, const SearchArgs& g, hipStream_t s) {
  const StepArgs a = search_keyed(in);
  return dispatch(v, [&](auto P, auto S) { return launch_waves(search_kernel<P, S>, g.num_playouts, s, a, g); });
}

hipError_t launch_search_bot(const Variant& v, const StepArgs& in, const SearchArgs& g, const BotArgs& bot, hipStream_t s) {
  const StepArgs a = search_keyed(in);
  return dispatch(v, [&](auto P, auto S) { return launch_waves(search_bot_kernel<P, S>, g.num_playouts, s, a, g, bot); });
}

}  // namespace gvec
