// gvec_bot.hpp — the scripted opponent's rule as device code (DESIGN.md §6 "Scripted opponent", restated by
// tests/_bot_reference.py): its one definition, shared by bot_kernel (gvec_bot_actions; gvec_kernels.hip) and by the playout
// search whose playouts play it (search_bot_kernel; gvec_search.hip).  All of it is forced inline.
#pragma once
#include "gvec_turn.hpp"

namespace gvec {

// Every plane below is packed like own[] / vis[] (row r of register k = player k*PPR + r), so one pass serves all players
// of a register.  A player sees a tile iff fog is off or its visibility bit is set; everything the rule reads about a tile
// is masked by that.

// the exploration draw of slot (env, player): independent of the agent's own h1 / h2 (other constants, a second round)
__device__ __forceinline__ uint32_t bot_mix_draw(uint32_t ek, uint32_t turn, uint32_t player) {
  const uint32_t h = amix((ek ^ 0x5851F42Du) + turn * 0x2C1B3C6Du + player * 0x297A2D39u);
  return amix(h ^ 0x1B873593u);
}

// the exploration mix: bit p <=> seat p plays the random agent's move this turn instead of the rule's (wave-uniform).
// Every lane calls it (a ballot); the caller skips it when random_permille is 0, where no bit can be set.
template <int MAXP>
__device__ __forceinline__ uint32_t bot_random_seats(uint32_t ek, uint32_t turn, int32_t random_permille) {
  const int lane = lane_id();
  const uint32_t h = bot_mix_draw(ek, turn, (uint32_t)lane);
  const bool rnd = lane < MAXP && (__umul24(h & 0xFFFFu, 1000u) >> 16) < (uint32_t)random_permille;
  return (uint32_t)__builtin_amdgcn_ballot_w64(rnd);
}

// max over the wave (every lane receives it)
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
  const int lane = lane_id();
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int src = (lane ^ off) << 2;
    const uint64_t o = ((uint64_t)bperm(src, (uint32_t)(v >> 32)) << 32) | bperm(src, (uint32_t)v);
    v = o > v ? o : v;
  }
  return v;
}

// "row r of x has a set bit", per lane (the same answer on every lane of the row)
template <typename BT>
__device__ __forceinline__ bool row_any(uint32_t x) {
  const unsigned long long bal = __builtin_amdgcn_ballot_w64(x != 0u);
  return row_slice<BT::ROWL>(bal, BT::row()) != 0u;
}

// wave-uniform bit set: bit k*PPR + r <=> row r of register k satisfied `flag` on some lane
template <typename BT>
__device__ __forceinline__ uint32_t rows_to_bits(bool flag, int k) {
  const unsigned long long bal = __builtin_amdgcn_ballot_w64(flag);
  uint32_t bits = 0u;
#pragma unroll
  for (int r = 0; r < BT::PPR; ++r)
    if (row_slice<BT::ROWL>(bal, r)) bits |= 1u << (k * BT::PPR + r);
  return bits;
}

// the bit string of source tiles s for which s + (direction d) lies in x (the legal mask's directions: up, right, down, left)
template <typename BT>
__device__ __forceinline__ uint32_t from_dir(const BT& b, uint32_t x, int d) {
  return d == 0 ? b.upW(x) : d == 1 ? b.dn1(x) : d == 2 ? b.dnW(x) : b.up1(x);
}

// The rule's moves of the seats in `movers` (wave-uniform; the caller has masked it to living seats of a live game) on the
// board b, whose legal planes (legal_planes<false>) are m.  Returns, in lane p, seat p's move as agent_sample returns one:
// t | d << 10 | 0x1000, or 0 when the seat is no mover or the rule finds it no move.
//   m IS OVERWRITTEN: every m[k][d] comes back masked by what the seat sees, and zero for a seat that is no mover.  A
//     caller that needs the legal planes afterwards takes its agent draw first, as bot_kernel does, or works on a copy.
//   b.larmy, the LDS army shadow, is written from the army registers here (army_to_lds) before it is read, and never
//     written otherwise.  turn_step does the same at the head of its action phase, fence included, and takes the armies
//     back into registers (army_from_lds) before it returns; no routine reads the shadow without having filled it first.
//     So the shadow carries nothing from turn to turn: what this function leaves there - the current armies - is as good to
//     the next turn_step as whatever the previous turn left, and what turn_step leaves (the armies as they stood before
//     production) is never read here.  The registers b.army[] are the state; they are only read.
//   Every cross-lane operation sits under a wave-uniform condition: movers != 0, need_bfs != 0, the BFS loop's `go`, the
//     seat loop's bit of movers.  The BFS loop ends at its fixpoint or when every source has been reached.
template <int MAXP, int NSLOT>
__device__ __forceinline__ uint32_t bot_sample(Turn<MAXP, NSLOT>& b, uint32_t (&m)[Turn<MAXP, NSLOT>::NR][4], uint32_t movers) {
  using B = Turn<MAXP, NSLOT>;
  constexpr int NR = B::NR, PPR = B::PPR, ROWL = B::ROWL;
  const int lane = lane_id();
  uint32_t bot_mine = 0u;  // lane p: t | d << 10 | 0x1000 (a move), as agent_sample returns it
  if (movers != 0u) {
    const bool fog = (b.hflags & HF_FOG) != 0u;
    b.army_to_lds();
    // ---- "army(s) - 1 > army(s + d)": a flat plane per direction, replicated (the ballots land in row 0, refresh_gt1's way)
    uint32_t mok[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int off = d == 0 ? -b.W : d == 1 ? 1 : d == 2 ? b.W : -1;
      uint32_t g = 0u;
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) {
        int idx = 64 * s + lane + off;
        idx = idx < 0 ? 0 : (idx > 64 * NSLOT - 1 ? 64 * NSLOT - 1 : idx);   // off the board: masked by the legal planes
        ballot_to_row0(g, __builtin_amdgcn_ballot_w64(b.army[s] - 1 > b.larmy[idx]), s);
      }
      mok[d] = B::replicate_row0(g);
    }
    uint32_t own_any = 0u;
#pragma unroll
    for (int k = 0; k < NR; ++k) own_any |= B::or_rows(b.own[k]);
    const uint32_t normal = b.valid & ~(b.gen | b.city | b.mtn);

    uint32_t seen[NR], sel[NR][4], cap_bits = 0u, need_bfs = 0u;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const bool mover = b.lane_flag(movers, k);
      seen[k] = fog ? b.vis[k] : b.valid;
      const uint32_t enemy = own_any & ~b.own[k] & seen[k];
      const uint32_t tgt = seen[k] & b.valid & ~b.mtn & ~b.own[k];
      const uint32_t t4 = b.gen & enemy, t3 = b.city & tgt, t2 = enemy & ~b.gen & ~b.city, t1 = tgt & ~own_any & ~b.city;
      uint32_t c4 = 0u, c3 = 0u, c2 = 0u, c1 = 0u;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        m[k][d] = mover ? (m[k][d] & seen[k]) : 0u;             // the sources p knows of, per direction
        const uint32_t c = m[k][d] & mok[d];
        c4 |= c & from_dir(b, t4, d);
        c3 |= c & from_dir(b, t3, d);
        c2 |= c & from_dir(b, t2, d);
        c1 |= c & from_dir(b, t1, d);
      }
      const bool h4 = row_any<B>(c4), h3 = row_any<B>(c3), h2 = row_any<B>(c2), h1 = row_any<B>(c1);
      const uint32_t best = h4 ? t4 : h3 ? t3 : h2 ? t2 : h1 ? t1 : 0u;   // the highest tier with a capture
#pragma unroll
      for (int d = 0; d < 4; ++d) sel[k][d] = m[k][d] & mok[d] & from_dir(b, best, d);
      const bool hc = h4 || h3 || h2 || h1;
      cap_bits |= rows_to_bits<B>(hc, k);
      need_bfs |= rows_to_bits<B>(mover && !hc && row_any<B>(m[k][0] | m[k][1] | m[k][2] | m[k][3]), k);
    }
    need_bfs &= movers & ~cap_bits;

    // ---- consolidation: BFS levels from the target set T, one 4-neighbour dilation per level
    if (need_bfs != 0u) {
      uint32_t reached[NR], front[NR], pass[NR], ownS[NR], pend[NR];
      bool any = false;
#pragma unroll
      for (int k = 0; k < NR; ++k) {
        const bool bfs = b.lane_flag(need_bfs, k);
        const uint32_t egen = b.gen & own_any & ~b.own[k] & seen[k];
        const uint32_t nrm = normal & seen[k] & ~b.own[k];
        const uint32_t hidden = fog ? (b.valid & ~seen[k]) : 0u;
        const uint32_t T = !bfs ? 0u : row_any<B>(egen) ? egen : row_any<B>(nrm) ? nrm : hidden;   // D = 0
        reached[k] = front[k] = T;
        pass[k] = b.valid & ~(seen[k] & b.mtn);
        ownS[k] = b.own[k] & seen[k];
        pend[k] = row_any<B>(T) ? (m[k][0] | m[k][1] | m[k][2] | m[k][3]) : 0u;   // sources not reached yet
#pragma unroll
        for (int d = 0; d < 4; ++d) sel[k][d] = bfs ? 0u : sel[k][d];
        any |= T != 0u;
      }
      // Level j + 1 = the passable, unreached 4-neighbours of level j.  A source s of level j + 1 is a candidate in direction
      // d when s + d is a level-j tile p owns (level 1 never qualifies: T holds no tile p owns).  Once every source has
      // been reached no later level can add one, so the loop ends there or at the fixpoint, whichever comes first.
      bool go = wave_any(any);
      while (go) {
        uint32_t grew = 0u, open = 0u;
#pragma unroll
        for (int k = 0; k < NR; ++k) {
          const uint32_t f = front[k];
          const uint32_t nxt = (f | b.upW(f) | b.dnW(f) | (b.up1(f) & b.ncol0) | (b.dn1(f) & b.ncolL)) & b.valid & pass[k] & ~reached[k];
          const uint32_t step = f & ownS[k];
#pragma unroll
          for (int d = 0; d < 4; ++d) sel[k][d] |= nxt & m[k][d] & from_dir(b, step, d);
          reached[k] |= nxt;
          front[k] = nxt;
          pend[k] &= ~nxt;
          grew |= nxt;
          open |= pend[k];
        }
        go = B::any_bit(grew) && B::any_bit(open);
      }
    }

    // ---- per player: the best key over the wave (captures: margin, consolidation: army; then lower tile, then direction)
    // The fence makes the margins below re-read the shadow.  Without it the compiler carries the NSLOT * 4 neighbour armies
    // of the margin planes above in registers across the BFS (bot_kernel<2,16>: 92 VGPRs and 5 waves instead of 63 and 7).
    wave_lds_fence();
#pragma unroll
    for (int p = 0; p < MAXP; ++p) {
      if (!((movers >> p) & 1u)) continue;
      const int k = p / PPR, rb = player_row<ROWL>(p);
      const bool cap = (cap_bits >> p) & 1u;
      uint64_t best = 0ull;
#pragma unroll
      for (int s = 0; s < NSLOT; ++s) {
        const uint32_t t = (uint32_t)(64 * s + lane);
        const uint64_t low = (uint64_t)((1023u - (t & 1023u)) << 2);
        if (cap) {
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const int off = d == 0 ? -b.W : d == 1 ? 1 : d == 2 ? b.W : -1;
            int idx = (int)t + off;
            idx = idx < 0 ? 0 : (idx > 64 * NSLOT - 1 ? 64 * NSLOT - 1 : idx);
            const uint64_t margin = (uint64_t)(uint32_t)(b.army[s] - 1 - b.larmy[idx]);
            const uint64_t key = gather(sel[k][d], s, rb) ? ((margin << 12) | low | (uint64_t)(3 - d)) : 0ull;
            best = key > best ? key : best;
          }
        } else {
          int dsel = -1;
#pragma unroll
          for (int d = 3; d >= 0; --d) dsel = gather(sel[k][d], s, rb) ? d : dsel;
          const uint64_t key = dsel >= 0 ? (((uint64_t)(uint32_t)b.army[s] << 12) | low | (uint64_t)(3 - dsel)) : 0ull;
          best = key > best ? key : best;
        }
      }
      best = wave_max_u64(best);
      if (best != 0ull) {
        const uint32_t t = 1023u - (uint32_t)((best >> 2) & 1023u), d = 3u - (uint32_t)(best & 3u);
        bot_mine = lane == p ? (t | (d << 10) | 0x1000u) : bot_mine;
      }
    }
  }
  return bot_mine;
}

}  // namespace gvec
