// gvec_mapgen.hip — the map generators: mapgen/generator.go on the counter RNG and on Go's math/rand.  One thread per board.
#include "gvec_launch.hpp"

namespace gvec {

// =========================================================================================
// map generator: algorithm and ratios of mapgen/generator.go:25-253 on the counter RNG.
// One thread per board (reset-time work, sequential by nature); mirrored by ora_mapgen.
// =========================================================================================
struct MRng {
  uint32_t key, ctr;
  __device__ uint32_t draw() { return fmix32(key + (ctr++) * 0x9E3779B9u); }
  __device__ int intn(int n) { return (int)__umulhi(draw(), (uint32_t)n); }
  __device__ int shuf(int n) { return intn(n); }
  __device__ void begin(const MapgenArgs& A, int i) {
    key = fmix32(env_key(A.seed_lo, A.seed_hi, (uint32_t)(A.first_index + i)) ^ 0x5BD1E995u);
    ctr = 0u;
  }
};

// Go's math/rand - rand.New(rand.NewSource(seed)), go 1.24 - one generator per thread: the additive lagged Fibonacci
// generator x[n] = x[n-607] + x[n-273] mod 2^64 seeded by the LCG x = 48271 x mod (2^31 - 1) XOR the 607-word table
// (derived by scripts/gen_go_rand_cooked.py, not copied).  The 607-word state lives in a caller-provided global buffer,
// word k of thread i at vec[k * stride] (threads seed in lock-step: coalesced).  Mirrored by the oracle's ora_gorand,
// which the reference's own seed-12345 vectors pin (tests/test_go_rand.py).
__device__ const uint64_t go_rng_cooked[607] = {
#include "go_rand_cooked.inc"
};
struct GoRng {
  uint64_t* vec;
  size_t stride;
  int tap, feed;
  static __device__ int32_t seedrand(int32_t x) {
    const int32_t hi = x / 44488, lo = x % 44488;
    x = 48271 * lo - 3399 * hi;
    return x < 0 ? x + 2147483647 : x;
  }
  __device__ void seed(int64_t s) {
    tap = 0;
    feed = 607 - 273;
    s %= 2147483647ll;
    if (s < 0) s += 2147483647ll;
    if (s == 0) s = 89482311ll;
    int32_t x = (int32_t)s;
    for (int i = -20; i < 607; ++i) {
      x = seedrand(x);
      if (i >= 0) {
        uint64_t u = (uint64_t)x << 40;
        x = seedrand(x);
        u ^= (uint64_t)x << 20;
        x = seedrand(x);
        u ^= (uint64_t)x;
        vec[(size_t)i * stride] = u ^ go_rng_cooked[i];
      }
    }
  }
  __device__ uint64_t int63() {
    if (--tap < 0) tap += 607;
    if (--feed < 0) feed += 607;
    const uint64_t x = vec[(size_t)feed * stride] + vec[(size_t)tap * stride];
    vec[(size_t)feed * stride] = x;
    return x & 0x7FFFFFFFFFFFFFFFull;
  }
  __device__ int intn(int n) {  // Intn -> Int31n
    if ((n & (n - 1)) == 0) return (int)(int63() >> 32) & (n - 1);
    const int32_t mx = (int32_t)(2147483647u - (2147483648u % (uint32_t)n));
    int32_t v = (int32_t)(int63() >> 32);
    while (v > mx) v = (int32_t)(int63() >> 32);
    return v % n;
  }
  __device__ int shuf(int n) {  // rand.go int31n (Shuffle): Lemire's multiply-shift on Uint32
    uint32_t v = (uint32_t)(int63() >> 31);
    uint64_t prod = (uint64_t)v * (uint64_t)(uint32_t)n;
    uint32_t low = (uint32_t)prod;
    if (low < (uint32_t)n) {
      const uint32_t thresh = (uint32_t)(-n) % (uint32_t)n;
      while (low < thresh) {
        v = (uint32_t)(int63() >> 31);
        prod = (uint64_t)v * (uint64_t)(uint32_t)n;
        low = (uint32_t)prod;
      }
    }
    return (int)(prod >> 32);
  }
  __device__ void begin(const MapgenArgs& A, int i) {
    vec = A.go_state + i;
    stride = (size_t)A.n;
    seed(A.go_seeds[i]);
  }
};

template <typename RNG>
__device__ __forceinline__ void mapgen_board(RNG& r, const MapgenArgs& A, int i) {
  const int w = A.in_width ? A.in_width[i] : A.max_w, h = A.in_height ? A.in_height[i] : A.max_h;
  const int players = A.in_players ? A.in_players[i] : A.max_p;
  A.width[i] = w;
  A.height[i] = h;
  A.players[i] = players;
  if (w < 1 || w > A.max_w || h < 1 || h > A.max_h || players < 1 || players > A.max_p) {
    atomicExch(A.status, GVEC_E_INVALID);
    return;
  }
  int32_t* army = A.army + (size_t)i * A.stride;
  int8_t* owner = A.owner + (size_t)i * A.stride;
  uint8_t* type = A.type + (size_t)i * A.stride;
  const int n = w * h;
  r.begin(A, i);
  for (int t = 0; t < A.stride; ++t) {
    army[t] = 0;
    owner[t] = -1;
    type[t] = GVEC_TILE_NORMAL;
  }
  // DefaultMapConfig (generator.go:25-47; config.go:198-200)
  int spacing = 5;
  if (spacing > w / 2 + h / 2) spacing = w / 2 + h / 2;
  const int veins = n / 50, min_len = 3, max_len = w / 4, city_ratio = 20, city_army = 40;
  for (int v = 0; v < veins; ++v) {  // placeMountains :77-142
    int cx = -1, cy = -1;
    for (int a = 0; a < 100; ++a) {
      const int x = r.intn(w), y = r.intn(h);
      const int idx = y * w + x;
      if (type[idx] == GVEC_TILE_NORMAL && owner[idx] == -1) {
        cx = x;
        cy = y;
        break;
      }
    }
    if (cx < 0) continue;
    type[cy * w + cx] = GVEC_TILE_MOUNTAIN;
    int len = min_len;
    if (max_len > min_len) len += r.intn(max_len - min_len + 1);
    for (int k = 1; k < len; ++k) {
      // dirs packed 2 bits each, N E S W = 0 1 2 3; rand.Shuffle = Fisher-Yates from the top (:117)
      uint32_t dirs = 0xE4u;  // [0]=0,[1]=1,[2]=2,[3]=3
      for (int a = 3; a > 0; --a) {
        const int j = r.shuf(a + 1);
        const uint32_t da = (dirs >> (2 * a)) & 3u, dj = (dirs >> (2 * j)) & 3u;
        dirs = (dirs & ~((3u << (2 * a)) | (3u << (2 * j))));
        dirs |= (dj << (2 * a)) | (da << (2 * j));
      }
      uint64_t cand = 0ull;  // candidate (x,y) pairs packed 10 bits each, in shuffled-direction order
      int nc = 0;
      for (int j = 0; j < 4; ++j) {
        const int d = (int)((dirs >> (2 * j)) & 3u);
        const int nx = cx + ((d == 1) - (d == 3)), ny = cy + ((d == 2) - (d == 0));
        if (nx >= 0 && nx < w && ny >= 0 && ny < h) {
          const int ni = ny * w + nx;
          if (type[ni] == GVEC_TILE_NORMAL && owner[ni] == -1) {
            cand |= (uint64_t)(uint32_t)(nx | (ny << 5)) << (10 * nc);
            nc++;
          }
        }
      }
      if (nc == 0) break;
      const int pick = r.intn(nc);
      const uint32_t c = (uint32_t)(cand >> (10 * pick)) & 1023u;
      cx = (int)(c & 31u);
      cy = (int)(c >> 5);
      type[cy * w + cx] = GVEC_TILE_MOUNTAIN;
    }
  }
  {  // placeCities :144-164
    const int want = n / city_ratio, max_attempts = want * 20;
    int placed = 0, attempts = 0;
    while (placed < want && attempts < max_attempts) {
      const int x = r.intn(w), y = r.intn(h);
      const int idx = y * w + x;
      if (owner[idx] == -1 && type[idx] == GVEC_TILE_NORMAL) {
        type[idx] = GVEC_TILE_CITY;
        army[idx] = city_army;
        placed++;
      }
      attempts++;
    }
  }
  int gx[GVEC_MAX_PLAYERS], gy[GVEC_MAX_PLAYERS];
  for (int pid = 0; pid < players; ++pid) {  // placeGenerals :166-253
    int placed_idx = -1;
    for (int a = 0; a < n && placed_idx < 0; ++a) {
      const int x = r.intn(w), y = r.intn(h);
      const int idx = y * w + x;
      if (owner[idx] != -1 || type[idx] != GVEC_TILE_NORMAL) continue;
      bool ok = true;
      for (int o = 0; o < pid; ++o) ok = ok && (abs(x - gx[o]) + abs(y - gy[o]) >= spacing);
      if (ok) placed_idx = idx;
    }
    for (int idx = 0; idx < n && placed_idx < 0; ++idx) {  // fallback scan :223-250
      if (owner[idx] != -1 || type[idx] != GVEC_TILE_NORMAL) continue;
      const int x = idx % w, y = idx / w;
      bool ok = true;
      for (int o = 0; o < pid; ++o) ok = ok && (abs(x - gx[o]) + abs(y - gy[o]) >= spacing);
      if (ok) placed_idx = idx;
    }
    if (placed_idx < 0) {
      atomicExch(A.status, GVEC_E_BOARD);
      return;
    }
    owner[placed_idx] = (int8_t)pid;
    army[placed_idx] = 2;
    type[placed_idx] = GVEC_TILE_GENERAL;
    gx[pid] = placed_idx % w;
    gy[pid] = placed_idx / w;
  }
}

__global__ void mapgen_kernel(MapgenArgs A) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= A.n) return;
  MRng r;
  mapgen_board(r, A, i);
}
// the same generator on Go's math/rand: board i = what game.NewEngine builds from GameConfig.Rng = rand.New(rand.NewSource(go_seeds[i]))
__global__ void mapgen_go_kernel(MapgenArgs A) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= A.n) return;
  GoRng r;
  mapgen_board(r, A, i);
}

hipError_t launch_mapgen(const MapgenArgs& a, hipStream_t s) {
  if (a.go_seeds) hipLaunchKernelGGL(mapgen_go_kernel, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(mapgen_kernel, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace gvec
