// gvec_search.hpp — what the playout kernels share (search_kernel and search_bot_kernel of gvec_search.hip, the expand pair of
// gvec_tree.hip): the playout index, the root and candidate loads, the invalid row, the candidate's slot of the ActVec and the
// eight terms, and the launch key.  They take and return plain values: a helper that returns the row through references, or
// one that holds the two early returns, compiles search_kernel to other instructions than before (all 18 instantiations;
// DESIGN.md §4.21), and these do not.  All of it is forced inline.
#pragma once
#include "gvec_turn.hpp"

namespace gvec {

// playout v's root i (returned) and candidate k
__device__ __forceinline__ int search_root_index(const SearchArgs& S, int v, int& k) {
  const int per_root = S.num_candidates * S.replicas;
  const int i = v / per_root;
  k = (v - i * per_root) / S.replicas;
  return i;
}
__device__ __forceinline__ int search_root_env(const SearchArgs& S, int i) { return S.root_envs ? uni(S.root_envs[i]) : i; }
__device__ __forceinline__ long long search_candidate(const SearchArgs& S, int i, int k) {
  return (long long)uni64((uint64_t)S.candidates[(size_t)i * S.num_candidates + k]);
}
// an INVALID row: all zeros, nothing is played
__device__ __forceinline__ void search_invalid_row(int32_t* out, int lane) {
  if (lane < GVEC_SEARCH_TERMS) out[lane] = 0;
}
// the seat is one the board has, and alive (alive implies below the env's player count)
template <int MAXP>
__device__ __forceinline__ bool search_seat_ok(uint32_t alive, int pl) {
  return pl >= 0 && pl < MAXP && ((alive >> (pl & 31)) & 1u) != 0u;
}
// the candidate's ActVec meta: the pass plays no move
__device__ __forceinline__ uint32_t search_meta(bool pass, bool half) { return pass ? 0u : (16u | (half ? 32u : 0u)); }
// turn 0 (cand: this lane is the seat's, on turn 0): the seat's slot is the candidate
template <typename AV>
__device__ __forceinline__ void search_override(AV& av, bool cand, uint32_t c_meta, int from, int tt) {
  av.meta = cand ? c_meta : av.meta;
  av.ft = cand ? from : av.ft;
  av.tt = cand ? tt : av.tt;
}
// the eight terms of the board as the playout left it after t turns
template <int MAXP, int NSLOT>
__device__ __forceinline__ void search_terms(const Turn<MAXP, NSLOT>& b, int32_t* out, int seat, int lane, int t) {
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

// the playout index is the key, whichever handle the roots live in
static inline StepArgs search_keyed(const StepArgs& in) {
  StepArgs keyed = in;
  keyed.env_base = 0;
  return with_seed_bases(keyed);
}

}  // namespace gvec
