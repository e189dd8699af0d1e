// gvec_arena.hip — the match arena's episode tally: finished games, outright wins, eliminations, lengths, returns and the
// pairwise placement table, counted per env from a self-play step's outputs (gvec_arena_update in generals_vec.h; DESIGN.md
// §4.18).
//
// One wavefront per env, four per workgroup, no LDS, no barrier and no atomic: every word of state belongs to one env, so
// the wave that owns the env is its only writer and every number is the same from run to run.  lane l < L carries column l
// (death, return, key); in the pair table lane p < L * L carries the pair (p / L, p % L).  An ordinary step loads 21 bytes and
// stores 12 per column.  Every branch is taken by the whole wave: the re-deal flag, the end of the episode, the cap and the
// truncation are per env, and their flags go through uni() so that the compiler branches on the scalar unit.  The only pass
// over board data is the land count of a truncated env - per surviving column, plane 1 of its observation with lane = tile,
// ARENA_TILES tiles per lane in flight, then a wave sum - which runs on the one step in max_turns where a batch dealt
// together is truncated together.
#include "gvec_launch.hpp"
#include "gvec_waves.hpp"

namespace gvec {

namespace {

constexpr int ARENA_TILES = 4;             // tiles per lane and pass of the land count: 1,024 tiles are four passes
constexpr int32_t SURVIVOR_KEY = 1 << 20;  // above every death step; + land <= 1,024

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void arena_update_kernel(gvec_arena_args P) {
  const int b = wave_item();
  if (b >= (int)P.rows) return;            // the whole wave leaves
  const int lane = lane_id();
  const int L = P.num_learners;
  const bool col = lane < L;
  const size_t at = (size_t)b * (size_t)L + (size_t)(col ? lane : 0);   // a lane past the columns reads column 0 and stores nothing

  if (P.reset && uni((int)P.reset[b]) != 0) {                           // a re-deal step is part of no game
    if (col) {
      P.death[at] = 0;
      P.ep_return[at] = 0.0;
    }
    if (lane == 0) P.ep_len[b] = 0;
    return;
  }

  const int ep_len = uni(P.ep_len[b]) + 1;
  const double ret = P.ep_return[at] + P.reward[at];
  int32_t death = P.death[at];
  const bool is_alive = P.alive ? P.alive[at] != 0 : true;
  if (death == 0 && !is_alive) death = ep_len;

  const bool terminated = uni((int)P.terminated[b]) != 0, truncated = uni((int)P.truncated[b]) != 0;
  if (!(terminated || truncated)) {                                     // the ordinary step
    if (col) {
      P.death[at] = death;
      P.ep_return[at] = ret;
    }
    if (lane == 0) P.ep_len[b] = ep_len;
    return;
  }

  const int games = uni(P.games[b]);
  if (!(P.games_cap > 0 && games == P.games_cap)) {
    // ---- keys: when a column died, or for a survivor how much land it holds at a truncation ----
    int32_t land = 0;
    if (P.obs && truncated && !terminated) {
      const int HW = P.width * P.height;
      const unsigned long long survivors = __builtin_amdgcn_ballot_w64(col && death == 0);
      for (int l = 0; l < L; ++l) {
        if (((survivors >> l) & 1ull) == 0ull) continue;                // wave-uniform: l and the ballot are scalars
        const float* plane = P.obs + ((size_t)b * (size_t)L + (size_t)l) * (size_t)P.obs_row_stride + (size_t)HW;
        uint32_t mine = 0u;
        for (int t0 = lane; t0 < HW; t0 += 64 * ARENA_TILES) {
          float v[ARENA_TILES];
#pragma unroll
          for (int u = 0; u < ARENA_TILES; ++u) v[u] = plane[min(t0 + 64 * u, HW - 1)];   // past the end: the last tile again, not counted
#pragma unroll
          for (int u = 0; u < ARENA_TILES; ++u) mine += (t0 + 64 * u < HW && v[u] == 0.5f) ? 1u : 0u;
        }
        // the loop above ends at a different trip count in lanes >= HW % 256: exec is whole again here
        const int32_t total = (int32_t)wave_sum(mine);
        if (lane == l) land = total;
      }
    }
    const int32_t key = death != 0 ? death : SURVIVOR_KEY + land;

    // ---- the pair table: lane p holds (i, j) = (p / L, p % L); both reads come before the logic ----
    const int i = min(lane / L, L - 1), j = lane % L;
    const int32_t key_i = __shfl(key, i, 64), key_j = __shfl(key, j, 64);
    if (lane < L * L && i != j) P.pair2[(size_t)b * (size_t)(L * L) + (size_t)lane] += key_i > key_j ? 2 : (key_i == key_j ? 1 : 0);

    if (lane == 0) {
      P.games[b] = games + 1;
      P.len_sum[b] += (int64_t)ep_len;
    }
    if (col) {
      const int winner = (int)P.winner[b];
      P.wins[at] += winner == P.player_ids[lane] ? 1 : 0;
      P.eliminated[at] += death != 0 ? 1 : 0;
      P.ret_sum[at] += ret;
    }
  }
  if (col) {                                                            // counted or not, the next step starts a new episode
    P.death[at] = 0;
    P.ep_return[at] = 0.0;
  }
  if (lane == 0) P.ep_len[b] = 0;
}

}  // namespace

hipError_t launch_arena_update(const gvec_arena_args& a, hipStream_t s) { return launch_waves(arena_update_kernel, a.rows, s, a); }

}  // namespace gvec
