// gvec_qtarget.hip — masked bootstrap targets from next observations: the legal-action mask of an observation, the scalar
// (Double) DQN target and the categorical (C51) target (gvec_obs_valid_mask, gvec_q_target, gvec_categorical_target in
// generals_vec.h).
//
// One wavefront per row, four per workgroup, no barrier between them (each wave owns its slice of LDS).
//   legal set  lane = tile (t = 64 s + lane): planes 1, 2 and 4 become two predicates, one ballot each; the ballot words are
//              the predicates' H*W-bit strings in LDS.  A tile's 5-bit code (bit d: action 5 t + d is legal) is its own source
//              bit and the passable bits of its four neighbours: legal_code, the one definition all three kernels use.
//   mask       the codes go to LDS as bytes; lane = output dword reads four of them back.  A row of 5 H W bytes starts at any
//              address, so a head and a tail of at most three bytes are stored singly.
//   scalar     lane = tile loads the at most five legal q_select values of its tile and nothing else; the running
//              (value, index) pairs meet in wave_argmax.  Lane 0 then loads q_eval[a*] and writes the row.
//   categorical the legal indices are compacted in ascending order into LDS (a prefix sum of the codes' popcounts per slot);
//              the loop over them runs lane = atom, QT_UNROLL actions' loads issued before the first one's reductions; the
//              projection reads p* and b lane by lane (v_readlane) in ascending j.
// Every reduction is a fixed xor butterfly (gvec_device.hpp): the same input gives the same bits.
#include <math.h>

#include "gvec_launch.hpp"
#include "gvec_waves.hpp"

namespace gvec {

namespace {

constexpr int QT_PRED_DW = 32;                   // 1,024 bits: GVEC_MAX_DIM squared
constexpr int QT_MAX_TILES = 32 * 32;
constexpr int QT_MAX_LEGAL = 5 * QT_MAX_TILES;   // every action of the largest board
constexpr int QT_UNROLL = 4;                     // atom rows in flight in the categorical loop

// ---- the legal set of an observation (generals_vec.h "masked Q targets") ----
// L[0 .. 31]: source bits (plane 1 == 0.5 and plane 2 > 0.09), L[32 .. 63]: passable bits (plane 4 == 0); bit t = tile t.
// Wave-uniform control flow only (ballots).  The words beyond the board's last slot are zero.
__device__ __forceinline__ void legal_planes(const float* __restrict__ o, int HW, uint32_t* L) {
  const int lane = lane_id(), slots = (HW + 63) >> 6;
  L[lane] = 0u;                                  // both planes; a wave's LDS writes land in order
  for (int s = 0; s < slots; ++s) {
    const int t = 64 * s + lane;
    const bool in = t < HW;
    const float v1 = in ? o[HW + t] : 0.0f, v2 = in ? o[2 * HW + t] : 0.0f, v4 = in ? o[4 * HW + t] : 1.0f;
    const unsigned long long src = __builtin_amdgcn_ballot_w64(in && v1 == 0.5f && v2 > 0.09f);
    const unsigned long long pas = __builtin_amdgcn_ballot_w64(in && v4 == 0.0f);
    if (lane == 0) {
      L[2 * s] = (uint32_t)src;
      L[2 * s + 1] = (uint32_t)(src >> 32);
      L[QT_PRED_DW + 2 * s] = (uint32_t)pas;
      L[QT_PRED_DW + 2 * s + 1] = (uint32_t)(pas >> 32);
    }
  }
  wave_lds_fence();
}
__device__ __forceinline__ uint32_t plane_bit(const uint32_t* plane, int t) { return (plane[t >> 5] >> (t & 31)) & 1u; }
// bit d < 4: the move from tile t in direction d (up, right, down, left) is legal; bit 4: the half move.  t < 1024; a tile
// beyond the board gets 0.  A neighbour off the board is not read (the index falls back to t itself).
__device__ __forceinline__ uint32_t legal_code(const uint32_t* L, int t, int W, int H) {
  const int y = t / W, x = t - y * W;
  const bool in = y < H, up = in && y > 0, right = in && x < W - 1, down = in && y < H - 1, left = in && x > 0;
  const uint32_t* pass = L + QT_PRED_DW;
  const uint32_t m = (up ? plane_bit(pass, up ? t - W : t) : 0u) | (right ? plane_bit(pass, right ? t + 1 : t) << 1 : 0u) |
                     (down ? plane_bit(pass, down ? t + W : t) << 2 : 0u) | (left ? plane_bit(pass, left ? t - 1 : t) << 3 : 0u);
  const uint32_t code = plane_bit(L, t) ? m : 0u;
  return code ? code | 16u : 0u;
}

// ---- gvec_obs_valid_mask ----
constexpr int MASK_WAVE_DW = 2 * QT_PRED_DW + QT_MAX_TILES / 4;   // the predicates, then one code byte per tile

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void obs_valid_mask_kernel(gvec_obs_valid_mask_args P) {
  __shared__ uint32_t mask_lds[WAVES_PER_BLOCK * MASK_WAVE_DW];
  const long long r = wave_item64();
  if (r >= P.rows) return;                       // the whole wave leaves: everything below is wave-uniform control flow
  const int lane = lane_id(), W = P.width, H = P.height, HW = W * H, A = 5 * HW, slots = (HW + 63) >> 6;
  uint32_t* L = mask_lds + block_wave() * MASK_WAVE_DW;
  uint8_t* codes = reinterpret_cast<uint8_t*>(L + 2 * QT_PRED_DW);
  legal_planes(P.obs + (size_t)r * (size_t)P.obs_row_stride, HW, L);
  for (int s = 0; s < slots; ++s) {
    const int t = 64 * s + lane;                 // < 1024: the codes of the tiles beyond the board are 0
    codes[t] = (uint8_t)legal_code(L, t, W, H);
  }
  wave_lds_fence();
  auto byte_of = [&](int i) -> uint32_t {        // i < A
    const uint32_t t = (uint32_t)i / 5u;
    return ((uint32_t)codes[t] >> ((uint32_t)i - 5u * t)) & 1u;
  };
  uint8_t* __restrict__ out = P.mask + (size_t)r * (size_t)A;
  const int h = (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(out) & 3u)) & 3u);
  const int head = h < A ? h : A, dwords = (A - head) >> 2;
  uint32_t* outw = reinterpret_cast<uint32_t*>(out + head);
  for (int j = lane; j < dwords; j += 64) {
    const int i = head + 4 * j;
    outw[j] = byte_of(i) | (byte_of(i + 1) << 8) | (byte_of(i + 2) << 16) | (byte_of(i + 3) << 24);
  }
  if (lane < head) out[lane] = (uint8_t)byte_of(lane);
  const int i1 = head + 4 * dwords + lane;       // tail: at most three bytes
  if (i1 < A) out[i1] = (uint8_t)byte_of(i1);
}

// the row's discount: its own, or the scalar gamma
template <typename ARGS>
__device__ __forceinline__ float discount_of(const ARGS& P, long long r) { return P.discount ? P.discount[r] : P.gamma; }

// ---- gvec_q_target ----
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void q_target_kernel(gvec_q_target_args P) {
  __shared__ uint32_t q_lds[WAVES_PER_BLOCK * 2 * QT_PRED_DW];
  const long long r = wave_item64();
  if (r >= P.rows) return;
  const int lane = lane_id(), W = P.width, H = P.height, HW = W * H, slots = (HW + 63) >> 6;
  const size_t A = 5u * (size_t)HW;
  uint32_t* L = q_lds + block_wave() * 2 * QT_PRED_DW;
  legal_planes(P.next_obs + (size_t)r * (size_t)P.obs_row_stride, HW, L);
  const float* __restrict__ qs = (P.q_select ? P.q_select : P.q_eval) + (size_t)r * A;
  float best = NEG_INF;
  int pick = NO_INDEX;
  for (int s = 0; s < slots; ++s) {
    const int t = 64 * s + lane;
    const uint32_t code = legal_code(L, t, W, H);
    float v[5];
#pragma unroll
    for (int d = 0; d < 5; ++d) v[d] = ((code >> d) & 1u) ? qs[5 * t + d] : 0.0f;   // the legal entries, and no other
#pragma unroll
    for (int d = 0; d < 5; ++d) {
      const int i = 5 * t + d;
      if (((code >> d) & 1u) && (v[d] > best || (v[d] == best && i < pick))) {
        best = v[d];
        pick = i;
      }
    }
  }
  wave_argmax(best, pick);
  if (lane == 0) {
    const bool won = pick != NO_INDEX, boot = won && P.done[r] == 0;
    const float nv = boot ? P.q_eval[(size_t)r * A + (size_t)(won ? pick : 0)] : 0.0f;
    const float rw = P.reward[r];
    P.target[r] = boot ? __fadd_rn(rw, __fmul_rn(discount_of(P, r), nv)) : rw;
    P.next_action[r] = won ? (long long)pick : -1ll;
    if (P.next_value) P.next_value[r] = nv;
  }
}

// ---- gvec_categorical_target ----
constexpr int C51_WAVE_DW = 2 * QT_PRED_DW + QT_MAX_LEGAL / 2;   // the predicates, then the legal indices as uint16

// softmax over the wave's first N lanes of x (the others hold -inf and get 0)
__device__ __forceinline__ float wave_softmax(float x, bool on) {
  const float m = wave_max(x);
  const float e = on ? expf(x - m) : 0.0f;
  return e / wave_sum(e);
}

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void categorical_target_kernel(gvec_categorical_target_args P) {
  __shared__ uint32_t c51_lds[WAVES_PER_BLOCK * C51_WAVE_DW];
  // not wave_item64(): with the row index wave-uniform the 16,384-row shapes of scripts/bench_qtarget.py measured 0.6-0.9 %
  // slower than the parent in each of three parent / result / parent runs (profiles/learner_units_ab.json), so this
  // kernel keeps the per-lane spelling
  const int wave = block_wave();
  const long long r = (long long)blockIdx.x * WAVES_PER_BLOCK + wave;
  if (r >= P.rows) return;
  const int lane = lane_id(), W = P.width, H = P.height, HW = W * H, slots = (HW + 63) >> 6, N = P.num_atoms;
  const size_t AN = 5u * (size_t)HW * (size_t)N;
  const bool on = lane < N;
  const float vmin = P.v_min, vmax = P.v_max, delta = (vmax - vmin) / (float)(N - 1);
  const float z = __fadd_rn(vmin, __fmul_rn((float)lane, delta));
  const float rw = P.reward[r];
  int pick = NO_INDEX;
  if (uni((int)P.done[r]) == 0) {                // wave-uniform: a done row reads neither its observation nor any logits
    uint32_t* L = c51_lds + wave * C51_WAVE_DW;
    uint16_t* list = reinterpret_cast<uint16_t*>(L + 2 * QT_PRED_DW);
    legal_planes(P.next_obs + (size_t)r * (size_t)P.obs_row_stride, HW, L);
    // compaction: the legal indices in ascending order
    int count = 0;
    for (int s = 0; s < slots; ++s) {
      const int t = 64 * s + lane;
      const uint32_t code = legal_code(L, t, W, H);
      const uint32_t n = (uint32_t)__builtin_popcount(code), incl = wave_scan_add(n);
      int at = count + (int)(incl - n);          // at + n <= 5 * (64 s + lane + 1) <= QT_MAX_LEGAL
#pragma unroll
      for (int d = 0; d < 5; ++d)
        if ((code >> d) & 1u) list[at++] = (uint16_t)(5 * t + d);
      count += (int)rdlane(incl, 63);
    }
    wave_lds_fence();
    // Q_i = sum_j softmax(logits_select[i])_j z_j over the legal i
    const float* __restrict__ sel = (P.logits_select ? P.logits_select : P.logits_eval) + (size_t)r * AN;
    float best = NEG_INF;
    for (int k0 = 0; k0 < count; k0 += QT_UNROLL) {
      int a[QT_UNROLL];
      float x[QT_UNROLL];
#pragma unroll
      for (int u = 0; u < QT_UNROLL; ++u) {      // the loads of QT_UNROLL actions first (the last group repeats its last action)
        const int k = k0 + u < count ? k0 + u : count - 1;
        a[u] = uni((int)list[k]);
        x[u] = on ? sel[(size_t)a[u] * (size_t)N + (size_t)lane] : NEG_INF;
      }
      float q[QT_UNROLL];
#pragma unroll
      for (int u = 0; u < QT_UNROLL; ++u) q[u] = wave_sum(wave_softmax(x[u], on) * z);   // independent chains: they interleave
#pragma unroll
      for (int u = 0; u < QT_UNROLL; ++u) {      // a repeated last action changes nothing: same value, same index
        if (q[u] > best || (q[u] == best && a[u] < pick)) {
          best = q[u];
          pick = a[u];
        }
      }
    }
  }
  // the projection: p* over the support moved by (reward, discount), or the point mass at the clamped reward
  pick = uni(pick);
  const bool boot = pick != NO_INDEX;
  float p = lane == 0 ? 1.0f : 0.0f, tz = rw;
  if (boot) {
    const float xe = on ? P.logits_eval[(size_t)r * AN + (size_t)pick * (size_t)N + (size_t)lane] : NEG_INF;
    p = wave_softmax(xe, on);
    tz = __fadd_rn(rw, __fmul_rn(discount_of(P, r), z));
  }
  tz = tz < vmin ? vmin : (tz > vmax ? vmax : tz);
  float b = (tz - vmin) / delta;
  const float top = (float)(N - 1);
  b = b < 0.0f ? 0.0f : (b > top ? top : b);     // rounding may leave b a few ulps beyond the last atom
  const float k = (float)lane;
  float acc = 0.0f;
  for (int j = 0; j < N; ++j) {
    const float w = 1.0f - fabsf(rdlane(b, j) - k);
    acc = acc + rdlane(p, j) * (w > 0.0f ? w : 0.0f);
  }
  if (on) P.m[(size_t)r * (size_t)N + (size_t)lane] = acc;
  if (lane == 0) P.next_action[r] = boot ? (long long)pick : -1ll;
}

}  // namespace

hipError_t launch_obs_valid_mask(const gvec_obs_valid_mask_args& a, hipStream_t s) { return launch_waves(obs_valid_mask_kernel, a.rows, s, a); }
hipError_t launch_q_target(const gvec_q_target_args& a, hipStream_t s) { return launch_waves(q_target_kernel, a.rows, s, a); }
hipError_t launch_categorical_target(const gvec_categorical_target_args& a, hipStream_t s) {
  return launch_waves(categorical_target_kernel, a.rows, s, a);
}

}  // namespace gvec
