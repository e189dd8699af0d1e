// gvec_gym_emit.hpp — gym_emit: the observation and mask stores observe_kernel (gvec_experience.hip) and the gym kernels
// (gvec_gym.hip) share.  Forced inline.
#pragma once
#include "gvec_launch.hpp"
#include "gvec_packed.hpp"

namespace gvec {

// The observation and mask of one env, from replicated flat planes (row 0 is read) of either board layout: `seen` what
// the proto shows as visible, own_p / own_any the learner's and anybody's tiles, m0..m3 the four direction planes of
// _get_valid_actions_mask and `many` their OR (index 4: "a half move is valid iff a full move is").  ms: this wave's
// LDS stage of (NSLOT*64*5 + 15)/16*16 bytes.
template <int NSLOT, typename BT>
__device__ __forceinline__ void gym_emit(const BT& b, uint32_t seen, uint32_t own_p, uint32_t own_any, uint32_t m0, uint32_t m1, uint32_t m2,
                                         uint32_t m3, uint32_t many, float tc, float* obs, uint8_t* mask, uint8_t* ms, int stride) {
  const int lane = lane_id();
  const uint32_t a0 = (uint32_t)(reinterpret_cast<uintptr_t>(obs) >> 2);
  if (((a0 | (uint32_t)stride) & 3u) != 0u) {
    // Planes of W*H floats that do not even start on 16-byte boundaries (odd W*H - 15x15: 900 bytes at multiples of 900;
    // 25x25: 2,500): a store of "tiles 64s .. 64s+63" begins anywhere in a line, and such stores leave at a third of the rate
    // of aligned ones (65,536 envs: the nine planes of 25x25 took 0.53 ms, those of 32x32 - 1.6x the bytes - 0.21).  So every
    // store covers an ALIGNED window of 64 floats instead, lane l of window k holding tile 64k - sh + l of its plane (sh: the
    // plane's dword offset inside its 256-byte line), whose bits come with the same ds_bpermute a slot's would: 25x25 0.77 ->
    // 0.47 ms, 15x15 0.256 -> 0.232.  (Planes on 16-byte boundaries are better off with the stores below - 10x10 0.140 vs
    // 0.162 ms this way, 20x20 0.260 vs 0.283 - whose per-slot bits all nine planes share.)
    auto at = [&](uint32_t plane, int t) { return __builtin_amdgcn_ubfe(bperm((t >> 5) << 2, plane), (uint32_t)(t & 31), 1u) != 0u; };
    auto emit = [&](int p, auto&& value) {
      float* base = obs + (size_t)p * (size_t)stride;
      const int sh = (int)((a0 + (uint32_t)p * (uint32_t)stride) & 63u);
#pragma unroll
      for (int k = 0; k <= NSLOT; ++k) {
        if (64 * k - sh < stride) {                  // wave-uniform
          const int t = 64 * k - sh + lane;
          const bool ok = t >= 0 && t < stride;
          const int tt = ok ? t : 0;
          const float v = value(k, tt, sh, ok && tt < b.N);
          if (ok) st_stream<GVEC_NT_MASK>(base + t, v);
        }
      }
    };
    emit(0, [&](int, int t, int, bool in) { const bool vis = at(seen, t); return (vis && in) ? 1.0f : 0.0f; });          // :312-314
    emit(1, [&](int, int t, int, bool in) {                                                                          // :316-322 (owner -1 unless visible)
      const bool vis = at(seen, t), mine = at(own_p, t), owned = at(own_any, t);
      return (in && vis && mine) ? 0.5f : ((in && vis && owned) ? 1.0f : 0.0f);
    });
    emit(2, [&](int k, int t, int sh, bool in) {
      // the army of tile 64k - sh + l sits in slot k (lanes l >= sh) or k - 1 (l < sh), sh lanes further on
      const int from = ((lane - sh) & 63) << 2;
      const int32_t cur = (int32_t)bperm(from, (uint32_t)b.army[k < NSLOT ? k : NSLOT - 1]);
      const int32_t prv = (int32_t)bperm(from, (uint32_t)b.army[k > 0 ? k - 1 : 0]);
      const bool vis = at(seen, t);
      const int32_t army = (vis && in) ? ((lane >= sh) ? cur : prv) : 0;         // hidden and fogged tiles: army 0
      // np.log(army + 1) / 10.0 in float64, cast on store (:324-326)
      return (army > 0) ? (float)(log((double)army + 1.0) / 10.0) : 0.0f;
    });
    // (every at() is a ds_bpermute and reads zeros from lanes that sit out: never behind a lane-dependent `&&`)
    emit(3, [&](int, int t, int, bool in) {                                                                          // :328-336 one-hot type
      const bool g = at(b.gen, t), c = at(b.city, t), mt = at(b.mtn, t);
      return (in && !g && !c && !mt) ? 1.0f : 0.0f;
    });
    emit(4, [&](int, int t, int, bool in) { const bool mt = at(b.mtn, t); return (in && mt) ? 1.0f : 0.0f; });
    emit(5, [&](int, int t, int, bool in) { const bool c = at(b.city, t); return (in && c) ? 1.0f : 0.0f; });
    emit(6, [&](int, int t, int, bool in) { const bool g = at(b.gen, t); return (in && g) ? 1.0f : 0.0f; });
    emit(7, [&](int, int, int, bool) { return tc; });                                                                // the whole plane, like obs[7, :, :] = ...
    emit(8, [&](int, int, int, bool) { return 0.0f; });                                                              // left zero by the reference (:341-343)
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const int t = 64 * s + lane;
      const uint32_t k0 = gather(m0, s), k1 = gather(m1, s), k2 = gather(m2, s), k3 = gather(m3, s), k4 = gather(many, s);
      if (t < stride) {
        uint8_t* mk = ms + t * 5;
        mk[0] = (uint8_t)k0;
        mk[1] = (uint8_t)k1;
        mk[2] = (uint8_t)k2;
        mk[3] = (uint8_t)k3;
        mk[4] = (uint8_t)k4;
      }
    }
  } else if constexpr (NSLOT >= 7) {
    // Boards of more than 256 tiles whose planes are a multiple of four floats on 16-byte boundaries (20x20, 24x25, 32x32):
    // FOUR neighbouring tiles per lane.  (65,536 envs: 20x20 0.255 -> 0.241 ms; smaller boards leave too many lanes without
    // a quad - 10x10 0.144 -> 0.159, 16x16 0.184 -> 0.195 - and keep the per-slot form below.)  Their bits are one nibble
    // of a plane's dword - one ds_bpermute per plane and 256 tiles instead of one per 64 - their armies one 16-byte LDS read,
    // each of the nine stores a 1-KB run of the wave, and the twenty mask bytes of the four tiles five dwords into the stage.
    const int nq = stride >> 2;
    constexpr int QI = (NSLOT + 3) / 4;
    int32_t* as = reinterpret_cast<int32_t*>(ms);             // the stage first carries the armies, tile t at dword t
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) as[64 * s + lane] = b.army[s];
    wave_lds_fence();
    int4 a4[QI];
#pragma unroll
    for (int i = 0; i < QI; ++i) {
      const int q = lane + 64 * i;
      a4[i] = (q < nq) ? *reinterpret_cast<const int4*>(as + 4 * q) : make_int4(0, 0, 0, 0);
    }
    wave_lds_fence();                                         // ... and is free for the mask bytes from here on
#pragma unroll
    for (int i = 0; i < QI; ++i) {
      if (64 * i < nq) {                                      // wave-uniform: the bpermutes below need every lane
        const int q = lane + 64 * i;
        const bool ok = q < nq;
        const int qq = ok ? q : 0;
        const int from = (qq >> 3) << 2, sh4 = (qq & 7) << 2;
        const uint32_t n_vis = (bperm(from, seen) >> sh4) & 15u, n_mine = (bperm(from, own_p) >> sh4) & 15u;
        const uint32_t n_any = (bperm(from, own_any) >> sh4) & 15u, n_g = (bperm(from, b.gen) >> sh4) & 15u;
        const uint32_t n_c = (bperm(from, b.city) >> sh4) & 15u, n_mt = (bperm(from, b.mtn) >> sh4) & 15u;
        uint32_t kd[5];
        kd[0] = (bperm(from, m0) >> sh4) & 15u;
        kd[1] = (bperm(from, m1) >> sh4) & 15u;
        kd[2] = (bperm(from, m2) >> sh4) & 15u;
        kd[3] = (bperm(from, m3) >> sh4) & 15u;
        kd[4] = (bperm(from, many) >> sh4) & 15u;
        const int t0 = qq << 2, left = b.N - t0;              // a smaller board in a padded batch ends inside or before the quad
        const uint32_t n_in = left >= 4 ? 15u : (left <= 0 ? 0u : ((1u << left) - 1u));
        const uint32_t v = n_vis & n_in;
        if (ok) {
          const size_t n = (size_t)stride;
          auto put = [&](int p, float x, float y, float z, float w) {
            float4 o;
            o.x = x; o.y = y; o.z = z; o.w = w;
            st_stream<GVEC_NT_MASK>(reinterpret_cast<u32x4*>(obs + p * n) + q, *reinterpret_cast<const u32x4*>(&o));
          };
          auto ones = [&](int p, uint32_t m) { put(p, (m & 1u) ? 1.0f : 0.0f, (m & 2u) ? 1.0f : 0.0f, (m & 4u) ? 1.0f : 0.0f, (m & 8u) ? 1.0f : 0.0f); };
          ones(0, v);                                                                                         // :312-314
          const uint32_t mine = v & n_mine, other = v & ~n_mine & n_any;                                      // :316-322 (owner -1 unless visible)
          put(1, (mine & 1u) ? 0.5f : ((other & 1u) ? 1.0f : 0.0f), (mine & 2u) ? 0.5f : ((other & 2u) ? 1.0f : 0.0f),
              (mine & 4u) ? 0.5f : ((other & 4u) ? 1.0f : 0.0f), (mine & 8u) ? 0.5f : ((other & 8u) ? 1.0f : 0.0f));
          // channel 2: np.log(army + 1) / 10.0 in float64, cast on store (:324-326); hidden and fogged tiles: army 0
          auto la = [](bool shown, int32_t a) { return (shown && a > 0) ? (float)(log((double)a + 1.0) / 10.0) : 0.0f; };
          put(2, la((v & 1u) != 0u, a4[i].x), la((v & 2u) != 0u, a4[i].y), la((v & 4u) != 0u, a4[i].z), la((v & 8u) != 0u, a4[i].w));
          ones(3, n_in & ~n_g & ~n_c & ~n_mt);                                                                // :328-336 one-hot type
          ones(4, n_in & n_mt);
          ones(5, n_in & n_c);
          ones(6, n_in & n_g);
          put(7, tc, tc, tc, tc);                                                                             // the whole plane, like obs[7, :, :] = ...
          put(8, 0.0f, 0.0f, 0.0f, 0.0f);                                                                     // left zero by the reference (:341-343)
          // mask byte 5 * tile + d of the quad's four tiles: twenty bytes = five dwords at byte 20 * q of the stage
          uint32_t w[5] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
          for (int bb = 0; bb < 20; ++bb) w[bb >> 2] |= ((kd[bb % 5] >> (bb / 5)) & 1u) << (8 * (bb & 3));
          uint32_t* mw = reinterpret_cast<uint32_t*>(ms) + 5 * q;
#pragma unroll
          for (int k = 0; k < 5; ++k) mw[k] = w[k];
        }
      }
    }
  
  } else {
  #pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const int t = 64 * s + lane;
      const bool vis = gather(seen, s) != 0u, mine = gather(own_p, s) != 0u, owned = gather(own_any, s) != 0u;
      const bool g = gather(b.gen, s) != 0u, c = gather(b.city, s) != 0u, mt = gather(b.mtn, s) != 0u;
      const uint32_t k0 = gather(m0, s), k1 = gather(m1, s), k2 = gather(m2, s), k3 = gather(m3, s), k4 = gather(many, s);
      const int32_t army = vis ? b.army[s] : 0;                                    // hidden and fogged tiles: army 0
      // channel 2: np.log(army + 1) / 10.0 in float64, cast on store (:324-326)
      const float la = (army > 0) ? (float)(log((double)army + 1.0) / 10.0) : 0.0f;
      if (t < stride) {
        const bool in = t < b.N;
        const size_t n = (size_t)stride;
        st_stream<GVEC_NT_MASK>(obs + 0 * n + t, (in && vis) ? 1.0f : 0.0f);                                // :312-314
        st_stream<GVEC_NT_MASK>(obs + 1 * n + t, (in && vis && mine) ? 0.5f : ((in && vis && owned) ? 1.0f : 0.0f));   // :316-322 (owner -1 unless visible)
        st_stream<GVEC_NT_MASK>(obs + 2 * n + t, in ? la : 0.0f);
        st_stream<GVEC_NT_MASK>(obs + 3 * n + t, (in && !g && !c && !mt) ? 1.0f : 0.0f);                    // :328-336 one-hot type
        st_stream<GVEC_NT_MASK>(obs + 4 * n + t, (in && mt) ? 1.0f : 0.0f);
        st_stream<GVEC_NT_MASK>(obs + 5 * n + t, (in && c) ? 1.0f : 0.0f);
        st_stream<GVEC_NT_MASK>(obs + 6 * n + t, (in && g) ? 1.0f : 0.0f);
        st_stream<GVEC_NT_MASK>(obs + 7 * n + t, tc);                                                       // the whole plane, like obs[7, :, :] = ...
        st_stream<GVEC_NT_MASK>(obs + 8 * n + t, 0.0f);                                                     // left zero by the reference (:341-343)
        uint8_t* mk = ms + t * 5;
        mk[0] = (uint8_t)k0;
        mk[1] = (uint8_t)k1;
        mk[2] = (uint8_t)k2;
        mk[3] = (uint8_t)k3;
        mk[4] = (uint8_t)k4;
      }
    }
  
  }
  wave_lds_fence();
  // the mask is five bytes per tile: laid out in LDS above and stored as whole 16-byte (or 4-byte) pieces of consecutive
  // lanes - five byte stores per lane and slot, each lane 5 bytes from its neighbour, held this kernel at 1.4 TB/s
  const int nbytes = 5 * stride;
  if ((nbytes & 15) == 0 && (reinterpret_cast<uintptr_t>(mask) & 15u) == 0u) {
    const u32x4* s4 = reinterpret_cast<const u32x4*>(ms);
    u32x4* g4 = reinterpret_cast<u32x4*>(mask);
    for (int i = lane; i < (nbytes >> 4); i += 64) st_stream<GVEC_NT_MASK>(g4 + i, s4[i]);
  } else if ((nbytes & 3) == 0 && (reinterpret_cast<uintptr_t>(mask) & 3u) == 0u) {
    const uint32_t* s1 = reinterpret_cast<const uint32_t*>(ms);
    uint32_t* g1 = reinterpret_cast<uint32_t*>(mask);
    for (int i = lane; i < (nbytes >> 2); i += 64) st_stream<GVEC_NT_MASK>(g1 + i, s1[i]);
  } else {
    for (int i = lane; i < nbytes; i += 64) mask[i] = ms[i];
  }
}

}  // namespace gvec
