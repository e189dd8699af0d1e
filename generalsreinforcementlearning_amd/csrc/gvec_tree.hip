// gvec_tree.hip — the device code of the tree search below the root (generals_vec.h "tree search below the root"; DESIGN.md
// §4.24): gvec_search_expand's pair of playout kernels, which keep the board after their first turn as a new node, and the two
// walks (gvec_tree_select, gvec_tree_backup).  The tree is node-major device arrays ([nodes][n][C], [nodes][n]); neither walk
// has LDS or a barrier.
//   select  one wavefront per (row, column), lane = child slot of the node the walk stands on.  A node's five slot arrays are
//           one coalesced load each; sumN, nmax, the two softmax sums and the argmax are fixed xor butterflies over all 64
//           lanes - the lanes beyond C and the slots that are not open carry neutral values (count 0, weight 0, score -inf)
//           instead of sitting out - so the same input gives the same bits.  The walk is a chain of dependent loads, a node
//           per level; what hides it is the other waves (n * k of them).  Reads only.
//   backup  one wavefront per row, lane = column.  A column's walk touches the edges of its own root slot's subtree and
//           nothing else, so the lanes never meet: no atomics, no cross-lane traffic, and the replicas are added in order.
// Every index read from memory (a node id, a slot) is range-checked before it becomes an address, and both walks are
// bounded by the number of nodes: a malformed tree ends a walk, it does not leave the arrays.
#include <math.h>

#include "gvec_bot.hpp"
#include "gvec_dispatch.hpp"
#include "gvec_playout_score.hpp"
#include "gvec_search.hpp"
#include "gvec_turn.hpp"
#include "gvec_waves.hpp"

namespace gvec {

// ---- gvec_search_expand: search_kernel's and search_bot_kernel's playouts (gvec_search.hip), with replica 0's board after
// its first turn kept as an env of the destination arrays - the node a tree search adds below (root i, candidate k).  The store is rollout_kernel's tail
// (store_army, settle_lists, store_hdr, store_planes with types), and the two things a store changes in the registers -
// hflags (HF_WIDE, HF_LDIFF as the stored form has them) and the packed header words - are put back afterwards, so that the
// turns that follow play on what search_kernel plays on and the terms stay its terms bit for bit.  Kernels of their own, so
// that the instruction streams of search_kernel and search_bot_kernel stay what they were.
//   pair = i * K + k; only replica 0 (`first`) stores and writes status[pair]
//   the destination slot's lifetime counters (H_CNT_*) stay its own: they are read from it into the header register first
__device__ __forceinline__ void expand_status(const SearchKeepArgs& E, int pair, bool first, int lane, int32_t st) {
  if (E.status && first && lane == 0) E.status[pair] = st;
}
// after the first turn (wave-uniform): stores the board if the pair has a destination env, returns the status word
template <int MAXP, int NSLOT>
__device__ __forceinline__ int32_t expand_keep(Turn<MAXP, NSLOT>& b, const StepArgs& A, const SearchKeepArgs& E, int pair, int seat, uint32_t err) {
  const int lane = lane_id();
  const int child = E.child_envs ? uni(E.child_envs[pair]) : pair;
  const bool keep = E.hdr != nullptr && child >= 0 && child < E.num_envs;   // checked here: no host copy of the ids
  if (keep) {
    const uint32_t hflags = b.hflags, hv = b.hv;
    uint32_t* hdr = E.hdr + (size_t)child * HDR_DW;
    const uint32_t own = lane < HDR_DW ? hdr[lane] : 0u;
    const uint32_t cs = rdlane(own, H_CNT_STEPS), ca = rdlane(own, H_CNT_ABORT), cd = rdlane(own, H_CNT_DONE);
    hdr_set(b, H_CNT_STEPS, cs);
    hdr_set(b, H_CNT_ABORT, ca);
    hdr_set(b, H_CNT_DONE, cd);
    store_army(b, army_ref<NSLOT>(E.army16, E.army32, child));
    settle_lists(b);
    b.store_hdr(hdr, err);
    b.store_planes(E.rows + (size_t)child * A.row_dw, A.fd, A.row_dw, true);
    b.hflags = hflags;
    b.hv = hv;
  }
  const bool over = (b.hflags & HF_DONE) != 0u, dead = ((b.alive >> seat) & 1u) == 0u;
  return (keep ? 1 : 0) | (over ? 2 : 0) | (dead ? 4 : 0);
}
template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, (rollout_waves<MAXP, NSLOT>())) void search_expand_kernel(StepArgs A, SearchArgs S, SearchKeepArgs E) {
  __shared__ int32_t army_shadow[WAVES_PER_BLOCK][NSLOT * 64];
  using B = Turn<MAXP, NSLOT>;
  __shared__ uint32_t act_scratch[WAVES_PER_BLOCK][B::ACT_SCRATCH_DW];
  const int wave = block_wave(), lane = lane_id();
  const int v = wave_item();
  if (v >= S.num_playouts) return;
  int k;
  const int i = search_root_index(S, v, k);
  const int pair = i * S.num_candidates + k;
  const bool first = v == pair * S.replicas;
  const int env = search_root_env(S, i);
  const int pl = uni(S.root_players[i]);
  const long long a = search_candidate(S, i, k);
  int32_t* out = S.terms + (size_t)v * GVEC_SEARCH_TERMS;
  if (env < 0 || env >= A.num_envs) {   // wave-uniform
    search_invalid_row(out, lane);
    expand_status(E, pair, first, lane, 0);
    return;
  }
  B b;
  b.larmy = army_shadow[wave];
  b.lscr = act_scratch[wave];
  load_turn(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd, A.zeros);
  const bool seat_ok = search_seat_ok<MAXP>(b.alive, pl);
  const int seat = seat_ok ? pl : 0;
  const GymMove mv = gym_decode(b, gym_sources(b, turn_view(b, seat)), a, S.stride);
  const bool pass = a == (long long)GVEC_SEARCH_PASS;
  if (!seat_ok || (b.hflags & HF_DONE) || !(pass || mv.accepted)) {   // wave-uniform
    search_invalid_row(out, lane);
    expand_status(E, pair, first, lane, 0);
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
    const uint32_t err = b.turn_step(av, A, aborted);
    ++t;
    b.refresh_gt1();
    if (t == 1 && first) expand_status(E, pair, first, lane, expand_keep<MAXP, NSLOT>(b, A, E, pair, seat, err));   // wave-uniform
    b.template legal_planes<false>(m);
  }
  search_terms<MAXP, NSLOT>(b, out, seat, lane, t);
}
template <int MAXP, int NSLOT>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, (rollout_waves<MAXP, NSLOT>())) void search_expand_bot_kernel(StepArgs A, SearchArgs S, BotArgs G,
                                                                                                               SearchKeepArgs E) {
  __shared__ int32_t army_shadow[WAVES_PER_BLOCK][NSLOT * 64];
  using B = Turn<MAXP, NSLOT>;
  __shared__ uint32_t act_scratch[WAVES_PER_BLOCK][B::ACT_SCRATCH_DW];
  const int wave = block_wave(), lane = lane_id();
  const int v = wave_item();
  if (v >= S.num_playouts) return;
  int k;
  const int i = search_root_index(S, v, k);
  const int pair = i * S.num_candidates + k;
  const bool first = v == pair * S.replicas;
  const int env = search_root_env(S, i);
  const int pl = uni(S.root_players[i]);
  const long long a = search_candidate(S, i, k);
  int32_t* out = S.terms + (size_t)v * GVEC_SEARCH_TERMS;
  if (env < 0 || env >= A.num_envs) {   // wave-uniform
    search_invalid_row(out, lane);
    expand_status(E, pair, first, lane, 0);
    return;
  }
  B b;
  b.larmy = army_shadow[wave];
  b.lscr = act_scratch[wave];
  load_turn(b, A.hdr + (size_t)env * HDR_DW, A.rows + (size_t)env * A.row_dw, army_cref<NSLOT>(A.army16, A.army32, env), A.fd, A.zeros);
  const bool seat_ok = search_seat_ok<MAXP>(b.alive, pl);
  const int seat = seat_ok ? pl : 0;
  const GymMove mv = gym_decode(b, gym_sources(b, turn_view(b, seat)), a, S.stride);
  const bool pass = a == (long long)GVEC_SEARCH_PASS;
  if (!seat_ok || (b.hflags & HF_DONE) || !(pass || mv.accepted)) {   // wave-uniform
    search_invalid_row(out, lane);
    expand_status(E, pair, first, lane, 0);
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
    const uint32_t err = b.turn_step(av, A, aborted);
    ++t;
    b.refresh_gt1();
    if (t == 1 && first) expand_status(E, pair, first, lane, expand_keep<MAXP, NSLOT>(b, A, E, pair, seat, err));   // wave-uniform
    b.template legal_planes<false>(m);
  }
  search_terms<MAXP, NSLOT>(b, out, seat, lane, t);
}

hipError_t launch_search_expand(const Variant& v, const StepArgs& in, const SearchArgs& g, const SearchKeepArgs& e, hipStream_t s) {
  const StepArgs a = search_keyed(in);
  return dispatch(v, [&](auto P, auto S) { return launch_waves(search_expand_kernel<P, S>, g.num_playouts, s, a, g, e); });
}

hipError_t launch_search_expand_bot(const Variant& v, const StepArgs& in, const SearchArgs& g, const BotArgs& bot, const SearchKeepArgs& e,
                                    hipStream_t s) {
  const StepArgs a = search_keyed(in);
  return dispatch(v, [&](auto P, auto S) { return launch_waves(search_expand_bot_kernel<P, S>, g.num_playouts, s, a, g, bot, e); });
}

namespace {

constexpr int TREE_NOT_EXPANDED = -1, TREE_DEAD = -2;
constexpr double NEG_INF64 = -__builtin_inf();

__device__ __forceinline__ size_t tree_node_row(const gvec_tree& T, int node, int r) { return (size_t)node * (size_t)T.n + (size_t)r; }

// ---- gvec_tree_select ----
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void tree_select_kernel(gvec_tree_select_args P) {
  const gvec_tree& T = P.tree;
  const int item = wave_item();
  if (item >= T.n * P.k) return;                 // the whole wave leaves: everything below is wave-uniform control flow
  const int lane = lane_id(), C = T.num_slots;
  const int r = item / P.k;
  int s = P.slot ? uni(P.slot[item]) : item - r * P.k;
  int u = 0, depth = 0;
  long long action = GVEC_SEARCH_NONE;
  if (s < 0 || s >= C) {
    s = -1;
  } else {
    // the column's root edge is given; below it every edge is the rule's pick
    for (int step = 0; step < T.nodes; ++step) {
      const size_t edge = tree_node_row(T, u, r) * (size_t)C + (size_t)s;
      const int child = uni(T.child_node[edge]);
      if (child == TREE_NOT_EXPANDED) {          // the leaf edge: the candidate to expand
        action = uni_ll(T.child_action[edge]);
        break;
      }
      if (child < 0 || child >= T.nodes) {       // dead (the root's own edge only: a dead slot is never picked), or not a node
        s = -1;
        break;
      }
      u = child;
      depth += 1;
      s = -1;
      if ((uni(T.node_status[tree_node_row(T, u, r)]) & 2) != 0) break;   // terminal
      // lane = slot of u
      const size_t base = tree_node_row(T, u, r) * (size_t)C;
      long long a = GVEC_SEARCH_NONE;
      int node = TREE_DEAD, cnt = 0;
      double logit = 0.0, sum = 0.0;
      if (lane < C) {
        a = T.child_action[base + lane];
        node = T.child_node[base + lane];
        cnt = T.child_count[base + lane];
        logit = (double)T.child_logit[base + lane];
        sum = T.child_sum[base + lane];
      }
      const bool open = a != GVEC_SEARCH_NONE && node != TREE_DEAD;
      if (!wave_any(open)) break;                // no open slot (wave-uniform: a ballot)
      const int n_c = open ? cnt : 0;
      const int total = wave_sum_int(n_c), nmax = wave_max_int(n_c);
      const bool seen = open && n_c > 0;
      const double top = wave_max_f64(open ? logit : NEG_INF64);
      const double w = open ? exp(logit - top) : 0.0;   // pi up to its normaliser, which cancels below
      const double q = seen ? sum / (double)n_c : 0.0;
      const double value = T.node_value[tree_node_row(T, u, r)];
      double vmix = value;
      const double den = wave_sum(seen ? w : 0.0), num = wave_sum(seen ? w * q : 0.0);
      if (total != 0) vmix = (value + (double)total * (num / den)) / (1.0 + (double)total);
      const double qhat = seen ? q : vmix;
      const double z = logit + ((P.c_visit + (double)nmax) * P.c_scale) * ((qhat - P.q_lo) * P.q_inv_range);
      const double ztop = wave_max_f64(open ? z : NEG_INF64);
      const double e = open ? exp(z - ztop) : 0.0;
      const double esum = wave_sum(e);
      const double score = open ? e / esum - (double)n_c / (1.0 + (double)total) : NEG_INF64;
      s = uni(wave_argmax_index(score, open ? lane : NO_INDEX));
      if (s >= C) {                              // no score compares (a NaN logit or value): not a slot, never an address
        s = -1;
        break;
      }
    }
    // a walk that ran out of steps stands on an edge it has not looked at: nothing to expand
    if (action == GVEC_SEARCH_NONE && s >= 0) {
      const size_t edge = tree_node_row(T, u, r) * (size_t)C + (size_t)s;
      if (uni(T.child_node[edge]) != TREE_NOT_EXPANDED) s = -1;
    }
  }
  if (lane == 0) {
    P.leaf_node[item] = u;
    P.leaf_slot[item] = s;
    P.leaf_action[item] = s >= 0 ? action : (long long)GVEC_SEARCH_NONE;
    P.leaf_depth[item] = depth;
  }
}

// ---- gvec_tree_backup ----
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void tree_backup_kernel(gvec_tree_backup_args P) {
  const gvec_tree& T = P.tree;
  const int r = wave_item();
  if (r >= T.n) return;
  const int lane = lane_id(), C = T.num_slots, R = P.replicas;
  if (lane >= P.k) return;                       // no cross-lane operation below: a column is a lane on its own
  const size_t col = (size_t)r * (size_t)P.k + (size_t)lane;
  int u = P.leaf_node[col], s = P.leaf_slot[col];
  if (u < 0 || u >= T.nodes || s >= C) return;
  double g;
  if (s >= 0) {
    const int32_t* __restrict__ t = P.terms + col * (size_t)R * GVEC_SEARCH_TERMS;
    double sum = 0.0;
    int cnt = 0;
    for (int j = 0; j < R; ++j, t += GVEC_SEARCH_TERMS) {
      if (t[0] != 0) {
        sum = sum + playout_score(P, t);
        cnt += 1;
      }
    }
    const int st = P.status[col];
    const size_t edge = tree_node_row(T, u, r) * (size_t)C + (size_t)s;
    if ((st & 1) == 0 || cnt == 0) {
      T.child_node[edge] = TREE_DEAD;
      return;
    }
    const int v = P.new_node[col];
    if (v < 1 || v >= T.nodes) return;
    g = sum / (double)cnt;
    if (P.net_value) g = (1.0 - P.value_weight) * g + P.value_weight * (double)P.net_value[col];
    T.child_node[edge] = v;
    const size_t at = tree_node_row(T, v, r);
    T.node_value[at] = g;
    T.node_status[at] = 1 | ((st & 6) != 0 ? 2 : 0);
    T.node_parent[at] = u;
    T.node_slot[at] = s;
  } else {
    if (u == 0) return;
    const size_t at = tree_node_row(T, u, r);
    if ((T.node_status[at] & 2) == 0) return;    // stopped at a node without an open slot: nothing to back up
    g = T.node_value[at];
    s = T.node_slot[at];
    u = T.node_parent[at];
  }
  // from the leaf edge up to the root's, inclusive
  for (int step = 0; step < T.nodes; ++step) {
    if (u < 0 || u >= T.nodes || s < 0 || s >= C) return;
    const size_t edge = tree_node_row(T, u, r) * (size_t)C + (size_t)s;
    T.child_sum[edge] = T.child_sum[edge] + g;
    T.child_count[edge] = T.child_count[edge] + 1;
    if (u == 0) return;
    const size_t at = tree_node_row(T, u, r);
    s = T.node_slot[at];
    u = T.node_parent[at];
  }
}

}  // namespace

hipError_t launch_tree_select(const gvec_tree_select_args& a, hipStream_t s) {
  return launch_waves(tree_select_kernel, (long long)a.tree.n * a.k, s, a);
}

hipError_t launch_tree_backup(const gvec_tree_backup_args& a, hipStream_t s) { return launch_waves(tree_backup_kernel, a.tree.n, s, a); }

}  // namespace gvec
