// gvec_symmetry.hip — the eight symmetries of the board (D4), one per row: plane sets, the legal mask, action-indexed values
// and the action of a batch of transitions in one launch (gvec_obs_symmetry in generals_vec.h).
//
// One wavefront per row, four per workgroup, no barrier between them (each wave owns its slice of LDS).
//   the row    sym, the action and with them the half-move rule are wave-uniform (scalar loads, scalar compares): a sym out of
//              range and a half move that is not exact under sym turn the row's symmetry into the identity.  Lane 0 writes
//              applied and the transformed action.
//   planes     lane = DESTINATION tile (t' = 64 s + lane): the source tile is computed once per slot and serves every plane of
//              every set, so the stores are dense dwords.  The loads of a flip are the same dense runs reversed, straight from
//              global memory.  A transposed row (sym & 4) reads with stride W, every cache line of the plane per load.  In a
//              large launch of a large board (launch_obs_symmetry has the rule) it is staged instead, SYM_STAGE_PLANES planes at
//              a time: dense loads into LDS, board rows W | 1 dwords apart, so that the column reads that follow fall on
//              distinct banks.
//   values     lane = destination dword of the row of 5 H W.
//   mask       lane = destination dword too: four source bytes gathered, one dword stored.  A row of 5 H W bytes starts at any
//              address, so a head and a tail of at most three bytes are stored singly.  A staged row's bytes are gathered from a
//              dense copy in the same LDS slice.
// Values move as 32-bit (8-bit) integers: no float instruction touches them.
#include "gvec_launch.hpp"
#include "gvec_waves.hpp"

namespace gvec {

namespace {

// d -> d' under sym, two bits per direction, one byte per sym (generals_vec.h "board symmetries")
constexpr uint64_t sym_dirs(int s, uint64_t up, uint64_t right, uint64_t down, uint64_t left) {
  return (up | right << 2 | down << 4 | left << 6) << (8 * s);
}
constexpr uint64_t SYM_DIRS = sym_dirs(0, 0, 1, 2, 3) | sym_dirs(1, 0, 3, 2, 1) | sym_dirs(2, 2, 1, 0, 3) | sym_dirs(3, 2, 3, 0, 1) |
                              sym_dirs(4, 3, 2, 1, 0) | sym_dirs(5, 3, 0, 1, 2) | sym_dirs(6, 1, 2, 3, 0) | sym_dirs(7, 1, 0, 3, 2);
__device__ __forceinline__ int sym_dir(int s, int d) { return d == 4 ? 4 : (int)((SYM_DIRS >> (8 * s + 2 * d)) & 3u); }
__device__ __forceinline__ int sym_inverse(int s) { return s == 5 ? 6 : (s == 6 ? 5 : s); }

// the board of one launch: t / W for t < 1024 and W <= 32 is (t * (65536 / W + 1)) >> 16, exactly (the error of the
// reciprocal, at most W / 65536 per unit of t / W, stays below 1 / W)
struct SymBoard {
  int W, H;
  uint32_t recip;
  __device__ __forceinline__ int row_of(int t) const { return (int)(((uint32_t)t * recip) >> 16); }
  // g(x, y) of sym s: the flips, then the transpose (W == H where s has it)
  __device__ __forceinline__ int image(int s, int x, int y) const {
    if (s & 1) x = W - 1 - x;
    if (s & 2) y = H - 1 - y;
    return (s & 4) ? x * W + y : y * W + x;
  }
  // the tile that sym s moves to t: the steps of g undone in reverse order.  pitch: the dwords between two board rows where
  // the source is read (W in global memory)
  __device__ __forceinline__ int source(int s, int t, int pitch) const {
    const int ty = row_of(t), tx = t - ty * W;
    int x = (s & 4) ? ty : tx, y = (s & 4) ? tx : ty;
    if (s & 1) x = W - 1 - x;
    if (s & 2) y = H - 1 - y;
    return y * pitch + x;
  }
  __device__ __forceinline__ int source(int s, int t) const { return source(s, t, W); }
  // the direction a half move from (x, y) is played in: the first of up, right, down, left that stays on the board
  __device__ __forceinline__ int half_dir(int x, int y) const { return y > 0 ? 0 : (x < W - 1 ? 1 : (y < H - 1 ? 2 : 3)); }
};

// When the transposed rows of a launch go through LDS (measured both ways): the board is 13 wide or more - a
// plane of a smaller one is at most five cache lines, and strided loads of it cost no more than the trip through LDS - and
// the launch has 4,096 rows or more - a smaller one is bound by a wave's own latency, which staging lengthens.
constexpr int SYM_STAGE_MIN_DIM = 13;
constexpr long long SYM_STAGE_MIN_ROWS = 4096;
constexpr int SYM_STAGE_PLANES = 3;              // planes of a transposed row in LDS at a time: 12.4 KB per wave at 32x32
// a wave's slice of LDS: SYM_STAGE_PLANES planes of H rows, W | 1 dwords apart (square boards only: nothing else transposes)
__host__ __device__ inline int sym_stage_dwords(int W, int H) { return W == H ? SYM_STAGE_PLANES * H * (W | 1) : 0; }

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void obs_symmetry_kernel(gvec_obs_symmetry_args P, int staged) {
  extern __shared__ uint32_t sym_lds[];
  const long long r = wave_item64();
  if (r >= P.rows) return;                       // the whole wave leaves: everything below is wave-uniform control flow
  const int lane = lane_id(), W = P.width, H = P.height, HW = W * H, A = 5 * HW, slots = (HW + 63) >> 6;
  const SymBoard B{W, H, 65536u / (uint32_t)W + 1u};

  // ---- the row's symmetry ----
  int sym = uni((int)P.sym[r]);
  if (sym >= (W == H ? 8 : 4)) sym = 0;
  long long act = -1;
  bool act_in = false;
  int at = 0, ad = 0;                            // the action's tile and direction
  if (P.action_in) {
    act = uni_ll(P.action_in[r]);
    act_in = act >= 0 && act < (long long)A;
    if (act_in) {
      at = (int)((uint32_t)act / 5u);
      ad = (int)act - 5 * at;
      if (ad == 4) {                             // exact iff the half move from g(t) plays the image of the one from t
        const int y = B.row_of(at), x = at - y * W, gt = B.image(sym, x, y), gy = B.row_of(gt);
        if (B.half_dir(gt - gy * W, gy) != sym_dir(sym, B.half_dir(x, y))) sym = 0;
      }
    }
  }
  const int e = P.inverse ? sym_inverse(sym) : sym;      // out[g_e(t)] = in[t]
  const int back = sym_inverse(e);                       // a destination direction's source
  if (lane == 0) {
    if (P.applied) P.applied[r] = (uint8_t)sym;
    if (P.action_out) {
      const int y = B.row_of(at), x = at - y * W;
      P.action_out[r] = act_in ? (long long)(5 * B.image(e, x, y) + sym_dir(e, ad)) : act;
    }
  }

  // ---- plane sets: lane = destination tile ----
  const bool through_lds = staged && (e & 4);
  const int pitch = W | 1, plane_dw = H * pitch;
  uint32_t* stage = sym_lds + block_wave() * sym_stage_dwords(W, H);
#pragma unroll 1
  for (int k = 0; k < P.num_sets; ++k) {          // one copy of the code for the four sets
    const int planes = P.sets[k].planes;
    const uint32_t* __restrict__ in = reinterpret_cast<const uint32_t*>(P.sets[k].in) + (size_t)r * (size_t)P.sets[k].in_row_stride;
    uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(P.sets[k].out) + (size_t)r * (size_t)planes * (size_t)HW;
    if (!through_lds) {                          // flips, and every row of a small launch: straight from global memory
      for (int s = 0; s < slots; ++s) {
        const int t = 64 * s + lane;
        if (t < HW) {
          const int src = B.source(e, t);
#pragma unroll 8
          for (int p = 0; p < planes; ++p) out[p * HW + t] = in[p * HW + src];
        }
      }
      continue;
    }
    for (int p0 = 0; p0 < planes; p0 += SYM_STAGE_PLANES) {      // the transpose: through LDS
      const int n = planes - p0;                 // planes of this pass: min(n, SYM_STAGE_PLANES)
#pragma unroll 4
      for (int s = 0; s < slots; ++s) {
        const int t = 64 * s + lane;
        if (t < HW) {
          const int to = t + B.row_of(t) * (pitch - W);    // row y of the board starts at y * pitch
#pragma unroll
          for (int c = 0; c < SYM_STAGE_PLANES; ++c)
            if (c < n) stage[c * plane_dw + to] = in[(p0 + c) * HW + t];
        }
      }
      wave_lds_fence();
      for (int s = 0; s < slots; ++s) {
        const int t = 64 * s + lane;
        if (t < HW) {
          const int src = B.source(e, t, pitch);
#pragma unroll
          for (int c = 0; c < SYM_STAGE_PLANES; ++c)
            if (c < n) out[(p0 + c) * HW + t] = stage[c * plane_dw + src];
        }
      }
      wave_lds_fence();                          // the next pass overwrites what this one read
    }
  }

  // the source of element i < A of an action-indexed row
  auto source_of = [&](int i) -> int {
    const int t = (int)((uint32_t)i / 5u), d = i - 5 * t;
    return 5 * B.source(e, t) + sym_dir(back, d);
  };

  // ---- values: lane = destination dword ----
  if (P.values_in) {
    const uint32_t* __restrict__ in = reinterpret_cast<const uint32_t*>(P.values_in) + (size_t)r * (size_t)A;
    uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(P.values_out) + (size_t)r * (size_t)A;
#pragma unroll 4
    for (int i = lane; i < A; i += 64) out[i] = in[source_of(i)];
  }

  // ---- mask: lane = destination dword of four bytes ----
  if (P.mask_in) {
    const uint8_t* __restrict__ in = P.mask_in + (size_t)r * (size_t)A;
    uint8_t* __restrict__ out = P.mask_out + (size_t)r * (size_t)A;
    const int h = (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(out) & 3u)) & 3u);
    const int head = h < A ? h : A, dwords = (A - head) >> 2;
    uint32_t* outw = reinterpret_cast<uint32_t*>(out + head);
    auto gather = [&](const uint8_t* __restrict__ from) {
#pragma unroll 2
      for (int j = lane; j < dwords; j += 64) {
        const int i = head + 4 * j;
        const uint32_t b0 = from[source_of(i)], b1 = from[source_of(i + 1)], b2 = from[source_of(i + 2)], b3 = from[source_of(i + 3)];
        outw[j] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
      }
      if (lane < head) out[lane] = from[source_of(lane)];
      const int i1 = head + 4 * dwords + lane;   // tail: at most three bytes
      if (i1 < A) out[i1] = from[source_of(i1)];
    };
    if (through_lds) {                           // the transpose: from a dense copy in LDS (5 H W bytes fit in three planes)
      uint8_t* copy = reinterpret_cast<uint8_t*>(stage);
#pragma unroll 4
      for (int i = lane; i < A; i += 64) copy[i] = in[i];
      wave_lds_fence();
      gather(copy);
    } else {
      gather(in);
    }
  }
}

}  // namespace

hipError_t launch_obs_symmetry(const gvec_obs_symmetry_args& a, hipStream_t s) {
  const int staged = a.width == a.height && a.width >= SYM_STAGE_MIN_DIM && a.rows >= SYM_STAGE_MIN_ROWS;
  const size_t lds = staged ? (size_t)WAVES_PER_BLOCK * (size_t)sym_stage_dwords(a.width, a.height) * sizeof(uint32_t) : 0;
  return launch_waves(obs_symmetry_kernel, a.rows, lds, s, a, staged);
}

}  // namespace gvec
