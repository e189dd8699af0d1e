// gvec_device.hpp — CDNA4 (gfx950) device code of the batched Generals.io turn engine.
//
// One 64-lane wavefront owns one board ("env").  The board lives in registers in two
// layouts at once (DESIGN.md "Data layout"):
//
//   * FLAT domain — every bit-plane is the row-major bit string of the board (bit t = tile
//     t = y*W + x, the reference's index, core/board.go:108); lane i holds bits 32i..32i+31:
//       own[p]  tile.Owner == p                  (core/board.go:8)
//       lst[p]  tile in Players[p].OwnedTiles    (game/state.go:12; SURVEY H6 "plane L")
//       vis[p]  bit p of tile.VisibleBitfield    (core/board.go:11)
//       chg     GameState.ChangedTiles, vch GameState.VisibilityChangedTiles (state.go:29,33)
//       gen/city/mtn  tile.Type one-hot          (core/board.go:20-26)
//     Neighbours are funnel shifts of the string by 1 (x +- 1, with column guards) and by W
//     (y +- 1): a DPP wave shift + v_alignbit each.  Ownership algebra and the legal-move
//     predicate are plain ANDs.  13 lanes carry a 20x20 board, 32 lanes a 32x32 one.
//   * TILE domain — lane l, slot s holds Tile.Army of tile t = 64*s + l (int32, H12).
//     A flat plane reaches the tile domain with one ds_bpermute (dword 2s + (l>>5)) and a
//     bit-field extract at bit l&31: no per-tile coordinates are ever computed.
//
//       gt1     Tile.Army > 1 of the resident state (the army-dependent half of every legal-move
//               predicate: stored so the next launch need not rebuild it from the armies)
//       valid / ncol0 / ncolL / ok[4]   geometry masks and "the d-neighbour is on the board and not a
//               mountain": functions of the board size and the type planes only, computed once when a
//               board is imported and carried as constant planes (loading 364 bytes costs less than
//               the ~55 vector instructions that rebuild them: the step kernel is VALU-issue bound)
//
// Planes and armies are loaded straight into registers (plane p: lane i reads dword i; armies:
// 256 B per wave instruction); the planes block of one env is a contiguous, 16-byte aligned run.  Integer / bit work only: no MFMA
// anywhere (HBM-roofline kernel).
//
// This file holds the PLAIN layout (`Board`: one register per plane, used by the conversion and experience
// kernels) and everything both layouts share - the header record's unpack and pack, the army storage, the flat <-> tile domain crossings, the move-target planes, the list settlement and the
// variant geometry; the turn logic lives in gvec_packed.hpp (`PBoard`).
//
// Every routine cites the Go function it reproduces (paths relative to
// /root/reference/internal/game/).  Semantics are the plane re-statement derived in
// SURVEY.md section 8 (H1-H12); tests/ checks them bit-for-bit against oracle/.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/generals_vec.h"

// clang has no __builtin for v_writelane_b32: bind the LLVM intrinsic directly (value and lane select must be
// wave-uniform; the backend moves a run-time lane select to M0)
extern "C" __device__ int gvec_llvm_writelane(int value, int lane, int vdst_in) __asm("llvm.amdgcn.writelane.i32");

// Streaming (non-temporal) cache policy on the turn kernels' once-per-launch accesses, by class (bits):
// 1 loads, 2 mask stores, 4 plane stores, 8 army stores.  One-process A/B at 262,144 boards 20x20 4P: nt LOADS
// cost 12 %, nt stores gain 3-4 % (the stored lines need not displace what the next loads want).
#ifndef GVEC_NT
#define GVEC_NT 14
#endif
#define GVEC_NT_MASK 2
#define GVEC_NT_PLANE 4
#define GVEC_NT_ARMY 8
// 1: the streaming stores carry `sc1 nt` - written through, the line dropped from the XCD's L2 - instead of `nt` alone.
// scripts/microbench/copy_pattern2.hip, the step kernel's bytes as 16-byte-per-lane stores: nt 255 us, nt sc1 196 us,
// sc1 alone 290 us, no bits 280 us per 262,144 boards.  The compiler has no spelling for the pair short of `volatile`
// (which also serialises the stores), hence the inline assembly; nothing ever waits for these stores, and the one
// wait state a wide store's data registers need before they are rewritten is in the string.
#ifndef GVEC_SC1
#define GVEC_SC1 1
#endif

// What the per-turn load path (load_turn<true>: step and gym kernels) and its staged plane store leave out because it
// carries no information for the turn (bits; DESIGN.md 4.1 "Lean traffic"; one-process A/B per bit, scripts/ab_bench.py):
// 1: ok[4] is rebuilt from mtn / valid / ncol0 / ncolL instead of loaded      2: the dead half of an odd last army slot is
// not loaded      4: the staged plane store ends on a whole 16-byte chunk (no 1..3-dword tail instruction)
#ifndef GVEC_LEAN
#define GVEC_LEAN 7
#endif

// Which fixed-pattern cross-lane moves of the turn run on the vector ALU (v_permlane16/32_swap, DPP row_newbcast,
// v_readlane into a lane mask) instead of as an LDS round trip (ds_bpermute / ds_swizzle), per idiom (bits; DESIGN.md 4.1
// "Cross-lane moves"; one-process A/B per bit, scripts/ab_bench.py).  A cleared bit compiles the LDS spelling:
// 1: shared_plane / spread_shared (row r of a register to every row)      2: replicate_row0 (refresh_gt1, the ballot planes)
// 4: or_rows and multi_sum's lane^16 / lane^32 steps      8: row_last (a row's last lane to that row)
// 16: the boards' own gather / gather_mask - production, the list sums, army_sum (a flat plane's dwords 2s, 2s+1 as a lane mask)
// Both spellings of every idiom are always compiled (`*_lds`, `*_valu` below): selftest_kernel holds one to the other.
// Measured (262,144 boards 20x20 4P, four sessions, profiles/xlane_ab.json): every bit alone is within 2 % of the LDS build and
// inside its max-min spread (7-9 us of 218); bits 1 and 2 gain nothing alone (218.1 / 217.5 vs 218.2 us) and every combination
// with them measured slower than the same without (16+2: 221.5 vs 220.0, 4+8+16+2: 222.7 vs 218.8, all five: 222.0 us), so they
// default to off.  No setting clears the project's margin (twice the parent's spread): LDS instructions per wave fall as
// counted, the wave's life does not.
#ifndef GVEC_XLANE
#define GVEC_XLANE 28
#endif
#define GVEC_XL_SPREAD 1
#define GVEC_XL_ROW0 2
#define GVEC_XL_ORROWS 4
#define GVEC_XL_ROWLAST 8
#define GVEC_XL_GATHER 16

// The per-turn step kernel's straight-line path for the ORDINARY turn (bits; DESIGN.md 4.1 "Ordinary turn"; one-process A/B
// per bit, scripts/ab_bench.py).  A wave decides ONCE, from the header words the scalar cache hands it, whether its env is live,
// in narrow army form, with lists equal to ownership, stats in sync, at most one captured tile per player and few special
// tiles (PBoard::ordinary_turn) - and then runs an instantiation of the turn in which every guard on those facts is folded to
// its known answer.  0 compiles the parent's step_kernel; the fused rollout, gym, search and bot kernels never take the path.
// 1: the path itself      4: growth turns (turn % interval == 0) are not ordinary: the path folds `grow` to false as well
// (2 was production's gathers reading their lane mask one slot ahead of the select that consumes it: six `s_nop` fewer on
// the path, 1.2-2.0 us SLOWER than bit 1 alone in three sessions of three - measured and taken out)
// Measured (262,144 boards 20x20 4P, three sessions, profiles/ordturn_ab.json): see DESIGN.md 4.1 "Ordinary turn".
#ifndef GVEC_ORDTURN
#define GVEC_ORDTURN 5
#endif
#define GVEC_OT_PATH 1
#define GVEC_OT_NOGROW 4

// What the ORDINARY turn of the per-turn step kernel leaves where it is because the turn did not change it (bits; DESIGN.md
// 4.1 "Quiet planes"; one-process A/B per bit, scripts/ab_bench.py, profiles/quiet_ab.json).  0 compiles the parent's
// step_kernel; the general code of step_kernel and every other kernel move all their planes whatever the value.  No plane
// moves and no header bit is spent:
// 1: the staged plane store leaves out the `own` chunks of a turn that changed no owner (every writer of own[] - act_vector,
//    the sequential chain, eliminate's turnover - puts the tile into V: the test is any_bit(vch) at the store) and the `vis`
//    chunks of a turn whose fog update was the identity (fog off, or V empty at the load).  ONE store instruction as before:
//    the lanes of the chunks that stay do not take part in it.  It travels in the turn's ORD template argument, above
//    GVEC_ORDTURN's own bits.
// (2 was `vis` out of the early load burst, fetched by the ordinary path only when the fog update would use it.  With the
// wait where update_fog stands it measured 1.5-5.7 us SLOWER than bit 1 alone in six sessions and alone no faster than the
// parent; with the update split and applied right before the store 7-8 us slower than bit 1 alone and 2-3 us slower than
// the parent (alone: 5 us slower than the parent): measured and taken out)
#ifndef GVEC_QUIET
#define GVEC_QUIET 1
#endif
#define GVEC_QT_STORE 1
#define GVEC_OT_QSTORE 16

namespace gvec {

// The same knob as constants of a kernel variant (NSLOT 64-tile slots, FD = 2*NSLOT or - `odd` - 2*NSLOT-1 plane dwords):
// shared by the kernels and by gvec_step_traffic_bytes, which reports what they move.
// ok[4] is rebuilt except on full 32-lane rows (NSLOT = 16: two players per register, 32 dwords a plane), whose shifts each
// cost a column select more and whose largest gym kernel has no register left for them (it would spill).
constexpr bool lean_derive_ok(int nslot) { return (GVEC_LEAN & 1) != 0 && 2 * nslot < 64 / (nslot <= 7 ? 4 : 2); }
// an `odd` board has at most 32*(2*NSLOT-1) tiles: lanes 32..63 of an odd last army slot hold none
constexpr bool lean_half_last(int nslot, bool odd) { return (GVEC_LEAN & 2) != 0 && odd && (nslot & 1) != 0; }
// dwords of the GEN plane the staged plane store rewrites to end on a 16-byte boundary (mutable_planes = Planes<MAXP>::MUTABLE)
constexpr int lean_fold_dwords(int mutable_planes, int fd) { return (GVEC_LEAN & 4) != 0 ? ((mutable_planes * fd + 3) & ~3) - mutable_planes * fd : 0; }
// GVEC_XLANE per variant: no kernel may lose a wave per SIMD or gain scratch for it (scripts/kernel_regs.py, every kernel of
// the library against the LDS build).  A swap of a register with itself needs a second register for its other result; the
// largest variant - eight players on full 32-lane rows - has none left in its gym step kernel (bit 1 alone: 12 bytes of
// scratch, bit 4 alone: 8), and the eight-player one-slot rollout kernel, which spills already, spills more (bit 4: +12
// bytes, bit 16: +4): these two keep the LDS spelling of those idioms.
constexpr bool xlane_tight(int maxp, int nslot) { return maxp >= 8 && nslot <= 1; }
constexpr bool xlane_swaps_ok(int maxp, int nslot) { return !(maxp >= 8 && nslot >= 16) && !xlane_tight(maxp, nslot); }
constexpr bool xlane_spread(int maxp, int nslot) { return (GVEC_XLANE & 1) != 0 && xlane_swaps_ok(maxp, nslot); }
constexpr bool xlane_or_rows(int maxp, int nslot) { return (GVEC_XLANE & 4) != 0 && xlane_swaps_ok(maxp, nslot); }
constexpr bool xlane_gather(int maxp, int nslot) { return (GVEC_XLANE & 16) != 0 && !xlane_tight(maxp, nslot); }
// GVEC_ORDTURN per step_kernel variant, as the ORD argument of the turn's templates (0: the general code alone).  No variant
// may lose a wave per SIMD or gain scratch for carrying two instantiations of the turn, nor grow past 40 KB of code (the
// instruction cache is 64 KB for two CUs; only <4,7,true,true> was timed) - scripts/isa_diff.py against the GVEC_ORDTURN=0
// build, every step_kernel.  The kernels that read their actions (AGENT false) hold fewer registers than the agent's and
// the allocator spends the difference: from ten slots on, and with eight players from two, they would drop from 8 waves to
// 7, 6 or 5 (<2,16>: 24-28 bytes of scratch).  Of the agent's kernels <8,10> (6 -> 5 waves) and <8,2,odd> (8 -> 7) would
// lose a wave, <4,16>, <8,4>, <8,7> would be 42-50 KB and <8,16> 79 KB.  These keep the general code: 43 of 72 carry the path.
// NOT held: "no more VGPRs than the parent".  Below the 64 registers of 8 waves the allocator takes what is free: the
// action-reading kernels that carry the path go from 50-55 to 55-64, seven of the agent's gain one; the waves per SIMD stay.
constexpr bool ordturn_fits(int maxp, int nslot, bool agent, bool odd) {
  if (!agent) return maxp <= 4 ? nslot <= 7 : nslot <= 1;
  return maxp <= 2 || (maxp <= 4 ? nslot <= 10 : (nslot <= 2 && !(nslot == 2 && odd)));
}
constexpr int ordturn_bits(int maxp, int nslot, bool agent, bool odd) {
  return (GVEC_ORDTURN & GVEC_OT_PATH) != 0 && ordturn_fits(maxp, nslot, agent, odd) ? (GVEC_ORDTURN & (GVEC_OT_PATH | GVEC_OT_NOGROW)) : 0;
}
// GVEC_QUIET per step_kernel variant, as a bit of the same ORD argument (only where the variant carries the ordinary path).  The
// own / vis boundary of the staged block (MAXP * fd dwords) must lie on a 16-byte chunk: at MAXP = 2 with an odd fd it does
// not, and those variants keep the parent's store (no narrow store for the last own dwords was built).  Otherwise
// ordturn_fits' rule: no wave per SIMD lost, no scratch gained, under 40 KB of code (scripts/kernel_regs.py): all hold it.
constexpr bool quiet_fits(int maxp, int nslot, bool agent, bool odd) {
  return ordturn_fits(maxp, nslot, agent, odd) && (maxp * (2 * nslot - (odd ? 1 : 0))) % 4 == 0;
}
constexpr int quiet_bits(int maxp, int nslot, bool agent, bool odd) {
  if (ordturn_bits(maxp, nslot, agent, odd) == 0 || !quiet_fits(maxp, nslot, agent, odd)) return 0;
  return (GVEC_QUIET & GVEC_QT_STORE) != 0 ? GVEC_OT_QSTORE : 0;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ T ld_stream(const T* p) {
  if constexpr ((GVEC_NT & 1) != 0) return __builtin_nontemporal_load(p);
  return *p;
}
__device__ __forceinline__ void st_through(uint32_t* p, uint32_t v) { asm volatile("global_store_dword %0, %1, off sc1 nt" : : "v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ void st_through(uint16_t* p, uint16_t v) {
  asm volatile("global_store_short %0, %1, off sc1 nt" : : "v"(p), "v"((uint32_t)v) : "memory");
}
__device__ __forceinline__ void st_through(float* p, float v) { asm volatile("global_store_dword %0, %1, off sc1 nt" : : "v"(p), "v"(v) : "memory"); }
// gfx940-family hazard: a VMEM store of more than 64 bits needs 2 wait states before a VALU write of its data
// registers, and the compiler's hazard recognizer cannot see a store inside an asm string: `s_nop 1` (= 2 wait
// states) is the only protection.  tests/test_kernel_asm.py scans the generated code for every such store.
__device__ __forceinline__ void st_through(u32x4* p, u32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1 nt\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
}
template <int CLASS, typename T>
__device__ __forceinline__ void st_stream(T* p, T v) {
  if constexpr ((GVEC_NT & CLASS) != 0) {
    if constexpr (GVEC_SC1 != 0) st_through(p, v);
    else __builtin_nontemporal_store(v, p);
  } else {
    *p = v;
  }
}

// ---- resident record layout (per env) -------------------------------------------------
// hdr  : HDR_DW u32      planes : M*FD u32 (+pad to 4), plane-major [m][i]
// army : NARROW block, NSLOT*64 u16 (the default), or - header flag HF_WIDE - the env's block of the
//        int32 escape array, NSLOT*64 i32 (see "army storage" below)
constexpr int HDR_DW = 24;
enum : int {
  H_TURN = 0,     // GameState.Turn
  H_DIMS = 1,     // W | H<<8 | P<<16 | flags<<24   (flags: HF_* below)
  H_STATUS = 2,   // alive bits | last err<<16
  H_EPISODE = 3,  // re-deal counter (auto-reset)
  H_ARMYCNT = 4,  // [8] Player.ArmyCount
  H_GIDX = 12,    // [8] Player.GeneralIdx
  H_RECIPW = 20,  // ceil(65536 / W): exact t / W for t < 1024
  H_CNT_STEPS = 21,  // lifetime counters of this env slot (rollout statistics)
  H_CNT_ABORT = 22,
  H_CNT_DONE = 23
};
constexpr uint32_t HF_DONE = 1u, HF_FOG = 2u, HF_WIDE = 4u;
constexpr uint32_t HF_SETUP = 8u;  // transient: imported with init, performInitialSetup still to run (setup_kernel clears it)
// Bookkeeping of the turn engine (never part of the exported state; all three absent = the general paths):
constexpr uint32_t HF_SYNC = 16u;        // the player stats are exactly what a stats pass over the current lists and armies yields
                                         // (set by every pass, cleared by an aborted turn and by every state import): the next
                                         // pass may add the turn's deltas to ArmyCount instead of summing the board
constexpr uint32_t HF_VSMALL = 32u;      // VisibilityChangedTiles holds at most one tile per player (no turnover since it was cleared)
constexpr uint32_t HF_LDIFF = 128u;      // some player's OwnedTiles differ from what it owns (H6: after an aborted turn, until a pass heals
                                         // it): only then are the LST planes of the block authoritative - and read or written at all.
                                         // Clear: lists == ownership, the stored LST planes are stale.  Kept true by settle_lists().
constexpr uint32_t HF_FEWSPECIAL = 64u;  // 2*P + generals + cities <= N/5 (a function of the board): without growth or turnover a
                                         // turn's ChangedTiles cannot reach the full-pass threshold

// plane order inside the planes block: what every turn rewrites (OWN .. GT1, contiguous), what changes only when a
// board is imported or re-dealt (GEN .. OK[3]), and last the list planes, which most turns neither read nor write
// (HF_LDIFF)
template <int MAXP>
struct Planes {
  static constexpr int OWN = 0, VIS = MAXP, CHG = 2 * MAXP, VCH = 2 * MAXP + 1, GT1 = 2 * MAXP + 2,
                       GEN = 2 * MAXP + 3, CITY = 2 * MAXP + 4, MTN = 2 * MAXP + 5, VALID = 2 * MAXP + 6, NCOL0 = 2 * MAXP + 7,
                       NCOLL = 2 * MAXP + 8, OK = 2 * MAXP + 9 /* [4]: up, right, down, left */, LST = 2 * MAXP + 13,
                       COUNT = 3 * MAXP + 13, MUTABLE = 2 * MAXP + 3, SHARED = 13 /* CHG .. OK[3] */;
};

// Geometry of a kernel variant whose plane stride is a compile-time constant.  ODD: the planes are 2*NSLOT-1 dwords long
// (else 2*NSLOT).  GYM_STAGE_DW: the gym mask's LDS stage (5 bytes a tile, whole 16-byte chunks).
template <int MAXP_, int NSLOT_, bool ODD_>
struct VariantGeom {
  static constexpr int MAXP = MAXP_, NSLOT = NSLOT_;
  static constexpr bool ODD = ODD_;
  static constexpr int FD = 2 * NSLOT - (ODD ? 1 : 0);
  static constexpr int ROW_DW = (Planes<MAXP>::COUNT * FD + 3) / 4 * 4;
  static constexpr int GYM_STAGE_DW = (NSLOT * 64 * 5 + 15) / 16 * 4;
  static_assert(GYM_STAGE_DW >= NSLOT * 64, "the larger user of the gym step kernels' army shadow: the stage serves as both");
};

constexpr uint32_t KF_AGENT = 1u;      // sample actions on device instead of reading them
constexpr uint32_t KF_EMIT = 2u;       // write legal-action masks
constexpr uint32_t KF_AUTORESET = 4u;  // re-deal finished envs from the pool
constexpr uint32_t KF_BIGRATE = 32u;   // a production rate so large that one turn takes a narrow army past 24 bits (host: base_args)
constexpr uint32_t KF_LMVALID = 16u;   // args.legal already holds the masks of the current state

struct StepArgs {
  uint32_t* hdr;
  uint32_t* rows;    // the planes block
  uint32_t* army16;  // narrow armies, NSLOT*32 dwords per env
  int32_t* army32;   // wide escape, NSLOT*64 dwords per env
  const gvec_action* actions;  // [B][pstride] (ignored with KF_AGENT)
  gvec_action* actions_out;    // optional: where the agent records what it played
  int32_t* err;                // [B] or null
  uint32_t* legal;             // [B][pstride][mask_dw]
  const uint32_t* zeros;  // >= row_dw zero dwords: what the lanes outside a board's bit string load
  const uint32_t* pool_hdr;
  const uint32_t* pool_rows;
  const uint32_t* pool_army16;
  const int32_t* pool_army32;
  int32_t num_envs, fd, row_dw, mask_dw, pool_size;  // fd = dwords per plane = ceil(max tiles / 32)
  int32_t pstride;  // players per env in actions / legal buffers (gvec_config.max_players)
  int32_t prod_general, prod_city, prod_normal, interval;
  uint32_t interval_magic;  // ceil(2^32 / interval)
  int32_t turns, invalid_permille;
  uint32_t agent_noop, agent_half;  // gvec_set_agent_mix thresholds (of 65536)
  uint32_t flags, seed_lo, seed_hi, pool_seed_lo, pool_seed_hi;
  uint32_t seed_base, pool_seed_base;  // env_key_base of the two seeds: filled in by the launchers (with_seed_bases)
  int32_t env_base;                    // host side only: this handle's first env within its sharded batch (folded into the bases)
};

// ---- army storage ------------------------------------------------------------------------
// Tile.Army is a Go int (core/board.go:9).  On the device it is computed in int32 registers and
// stored in one of two forms, chosen per env at every store:
//   NARROW  u16, when every army of the board is in [0, 65535] (virtually always): two 64-tile slots
//           share a dword - dword 64k+l = army(slot 2k, lane l) | army(slot 2k+1, lane l) << 16 - so one
//           256-byte wave access moves 128 tiles; an odd last slot is 64 halfwords (one 128-byte line).
//           NSLOT*128 bytes per env: 896 B instead of 1,792 B at 20x20.
//   WIDE    int32 in the env's block of the escape array (header flag HF_WIDE), as soon as one army
//           leaves that range.  Exact for everything an int32 can hold; the env returns to NARROW at
//           the first store where it fits again.
// Nothing is ever clamped: the pair (flag, block) always holds the exact int32 value.
struct ArmyRef {
  uint32_t* n;  // this env's narrow block (NSLOT*32 dwords)
  int32_t* w;   // this env's wide block   (NSLOT*64 dwords)
};
struct ArmyCRef {
  const uint32_t* n;
  const int32_t* w;
  __device__ __forceinline__ ArmyCRef(const uint32_t* n_, const int32_t* w_) : n(n_), w(w_) {}
  __device__ __forceinline__ ArmyCRef(const ArmyRef& r) : n(r.n), w(r.w) {}
};
template <int NSLOT>
__device__ __forceinline__ ArmyRef army_ref(uint32_t* a16, int32_t* a32, int env) {
  return ArmyRef{a16 + (size_t)env * (NSLOT * 32), a32 + (size_t)env * (NSLOT * 64)};
}
template <int NSLOT>
__device__ __forceinline__ ArmyCRef army_cref(const uint32_t* a16, const int32_t* a32, int env) {
  return ArmyCRef(a16 + (size_t)env * (NSLOT * 32), a32 + (size_t)env * (NSLOT * 64));
}
// HALF_LAST (odd NSLOT only): the caller knows that the board has at most 32*(2*NSLOT-1) tiles, so lanes 32..63 of the
// last slot hold no tile - they are zero in memory from import or re-deal on, and every store writes zeros back - and read
// as zero without a load
template <int NSLOT, bool HALF_LAST = false>
__device__ __forceinline__ void army_load_narrow(int32_t (&army)[NSLOT], const uint32_t* n) {
  const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
  for (int k = 0; k < NSLOT / 2; ++k) {
    const uint32_t w = ld_stream(n + 64 * k + lane);
    army[2 * k] = (int32_t)(w & 0xFFFFu);
    army[2 * k + 1] = (int32_t)(w >> 16);
  }
  if constexpr ((NSLOT & 1) != 0) {
    if constexpr (HALF_LAST) {
      army[NSLOT - 1] = 0;
      if (lane < 32) army[NSLOT - 1] = (int32_t)ld_stream(reinterpret_cast<const uint16_t*>(n + 64 * (NSLOT / 2)) + lane);
    } else {
      army[NSLOT - 1] = (int32_t)ld_stream(reinterpret_cast<const uint16_t*>(n + 64 * (NSLOT / 2)) + lane);
    }
  }
}
template <int NSLOT>
__device__ __forceinline__ void army_load_wide(int32_t (&army)[NSLOT], const int32_t* w) {
  const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) army[s] = w[64 * s + lane];
}
// wave-uniform: every army of the board fits the narrow form (negative values have bit 31 set)
template <int NSLOT>
__device__ __forceinline__ bool army_fits_narrow(const int32_t (&army)[NSLOT]) {
  uint32_t m = 0u;
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) m |= (uint32_t)army[s];
  return __builtin_amdgcn_ballot_w64(m > 0xFFFFu) == 0ull;
}
template <int NSLOT>
__device__ __forceinline__ void army_store_narrow(const int32_t (&army)[NSLOT], uint32_t* n) {
  const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
  for (int k = 0; k < NSLOT / 2; ++k) st_stream<GVEC_NT_ARMY>(n + 64 * k + lane, (uint32_t)army[2 * k] | ((uint32_t)army[2 * k + 1] << 16));
  if constexpr ((NSLOT & 1) != 0) st_stream<GVEC_NT_ARMY>(reinterpret_cast<uint16_t*>(n + 64 * (NSLOT / 2)) + lane, (uint16_t)army[NSLOT - 1]);
}
template <int NSLOT>
__device__ __forceinline__ void army_store_wide(const int32_t (&army)[NSLOT], int32_t* w) {
  const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) w[64 * s + lane] = army[s];
}

// The two forms for any board type with army[] and hflags.  Whole 64-tile slots travel both ways (the padding beyond N
// holds zeros).  The narrow block is read unconditionally (its loads need not wait for the header); a WIDE env - rare -
// reads its escape block on top.  Needs hflags: call after load_hdr.
template <typename BT>
__device__ __forceinline__ void load_army(BT& b, const ArmyCRef& a) {
  army_load_narrow(b.army, a.n);
  if (b.hflags & HF_WIDE) army_load_wide(b.army, a.w);
}
// Chooses the form (and sets / clears HF_WIDE in hflags accordingly): call BEFORE store_hdr.  STAGED: the narrow block
// leaves through the board's LDS stage (PBoard::store_army_narrow_staged).
template <bool STAGED = false, typename BT>
__device__ __forceinline__ void store_army(BT& b, const ArmyRef& a) {
  if (army_fits_narrow(b.army)) {
    b.hflags &= ~HF_WIDE;
    if constexpr (STAGED) b.store_army_narrow_staged(a.n);
    else army_store_narrow(b.army, a.n);
  } else {
    b.hflags |= HF_WIDE;
    army_store_wide(b.army, a.w);
  }
}

// ---- wave primitives --------------------------------------------------------------------
// NOTE: ds_bpermute / DPP read 0 from lanes that are masked off in EXEC.  Every cross-lane
// helper below must therefore be called under wave-uniform control flow only.
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }

template <int CTRL, int RM = 0xf, int BM = 0xf>
__device__ __forceinline__ uint32_t dpp0(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, RM, BM, false);
}
// lane i receives lane i-1 (the 32 tiles before); lane 0 receives 0     [DPP wave_shr:1]
__device__ __forceinline__ uint32_t from_prev(uint32_t v) { return dpp0<0x138>(v); }
// lane i receives lane i+1 (the 32 tiles after); lane 63 receives 0     [DPP wave_shl:1]
__device__ __forceinline__ uint32_t from_next(uint32_t v) { return dpp0<0x130>(v); }

// inclusive prefix sum over the 64 lanes (row_shr 1/2/4/8, then row_bcast 15/31)
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) {
  v += dpp0<0x111>(v);
  v += dpp0<0x112>(v);
  v += dpp0<0x114>(v);
  v += dpp0<0x118>(v);
  v += dpp0<0x142, 0xa>(v);
  v += dpp0<0x143, 0xc>(v);
  return v;
}
// a * b + c on the low 24 bits of a and b, full rate.  Written as one instruction because the compiler
// otherwise splits it into v_mul_u32_u24 + a shared v_add3 (2.5 instead of 2 instructions per term).
__device__ __forceinline__ uint32_t mad24(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t d;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
__device__ __forceinline__ uint32_t rdlane(uint32_t v, int lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}
__device__ __forceinline__ float rdlane(float v, int lane) { return __uint_as_float(rdlane(__float_as_uint(v), lane)); }
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
// the signed form under a name of its own: an int64_t argument would not choose between two overloads
__device__ __forceinline__ long long uni_ll(long long v) { return (long long)uni64((uint64_t)v); }
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return rdlane(wave_scan_add(v), 63); }
__device__ __forceinline__ bool wave_any(bool c) { return __builtin_amdgcn_ballot_w64(c) != 0ull; }
// float reductions as fixed xor butterflies: every lane ends with the same value, and the same input gives the same bits
constexpr float NEG_INF = -__builtin_inff();  // what a masked-out entry holds, and the identity of wave_max
constexpr int NO_INDEX = 0x7FFFFFFF;          // wave_argmax's index of "no entry": loses every tie
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float o = __shfl_xor(x, off, 64);
    x = o > x ? o : x;
  }
  return x;
}
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off, 64);
  return x;
}
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off, 64);
  return x;
}
// ... in float64 and on counts, under names of their own (an overload would capture the existing calls with int arguments):
// the tree walks of gvec_tree.hip
__device__ __forceinline__ double wave_max_f64(double x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = __shfl_xor(x, off, 64);
    x = o > x ? o : x;
  }
  return x;
}
__device__ __forceinline__ int wave_max_int(int x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int o = __shfl_xor(x, off, 64);
    x = o > x ? o : x;
  }
  return x;
}
__device__ __forceinline__ int wave_sum_int(int x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off, 64);
  return x;
}
// the greatest float64 value, the lowest index among equals: every lane ends with the same index
__device__ __forceinline__ int wave_argmax_index(double v, int idx) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(v, off, 64);
    const int oi = __shfl_xor(idx, off, 64);
    const bool take = ov > v || (ov == v && oi < idx);
    v = take ? ov : v;
    idx = take ? oi : idx;
  }
  return idx;
}
// the greatest value, the lowest index among equals; every lane ends with the same pair
__device__ __forceinline__ void wave_argmax(float& v, int& idx) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const int oi = __shfl_xor(idx, off, 64);
    const bool take = ov > v || (ov == v && oi < idx);
    v = take ? ov : v;
    idx = take ? oi : idx;
  }
}
__device__ __forceinline__ uint32_t bperm(int byte_addr, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute(byte_addr, (int)v);
}
// ---- fixed-pattern moves between rows, on the vector ALU (GVEC_XLANE) ---------------------------------
// EXEC: ds_bpermute / ds_swizzle return 0 from a lane that is masked off; v_permlane16/32_swap and DPP row_newbcast leave the
// lanes of a masked-off lane's pair UNTOUCHED instead.  Every routine below must therefore run with EXEC full: at the top
// level of a kernel whose waves are whole, or under conditions that are wave-uniform in VALUE (header flags, kernel
// arguments, ballots) - which is what the LDS spellings already demanded (the NOTE above).  The builtins, never asm strings:
// the hazard recognizer pads a swap that follows a VALU write of its operands by itself.
struct LanePair {
  uint32_t a, b;
};
// v_permlane16_swap_b32 of (x, x): with x's four 16-lane rows [A, B, C, D], a = [A, A, C, C] and b = [B, B, D, D]
__device__ __forceinline__ LanePair swap16(uint32_t x) {
  const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
  return LanePair{(uint32_t)r[0], (uint32_t)r[1]};
}
// v_permlane32_swap_b32 of (x, x): with x's two halves [L, H], a = [L, L] and b = [H, H]
__device__ __forceinline__ LanePair swap32(uint32_t x) {
  const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  return LanePair{(uint32_t)r[0], (uint32_t)r[1]};
}
// Two values whose OR / sum is x[lane] (op) x[lane ^ D], D = 16 or 32: the lane's own and its partner's (LDS), or the pair's
// two values in an order that depends on the lane (a swap of x with itself) - any commutative op gives the same result.
template <int D>
__device__ __forceinline__ LanePair with_partner_lds(uint32_t x) {
  static_assert(D == 16 || D == 32, "lane ^ 16 or lane ^ 32");
  if constexpr (D == 16) return LanePair{x, (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, 0x401F)};
  return LanePair{x, bperm((lane_id() ^ 32) << 2, x)};
}
template <int D>
__device__ __forceinline__ LanePair with_partner_valu(uint32_t x) {
  static_assert(D == 16 || D == 32, "lane ^ 16 or lane ^ 32");
  if constexpr (D == 16) return swap16(x);
  return swap32(x);
}
template <int D, bool VALU>
__device__ __forceinline__ LanePair with_partner(uint32_t x) {
  if constexpr (VALU) return with_partner_valu<D>(x);
  return with_partner_lds<D>(x);
}
// row r (ROWL lanes: r < 64 / ROWL, a compile-time constant once inlined) of x in every row
template <int ROWL>
__device__ __forceinline__ uint32_t row_to_all_lds(uint32_t x, int r) {
  return bperm((r * ROWL + (lane_id() & (ROWL - 1))) << 2, x);
}
template <int ROWL>
__device__ __forceinline__ uint32_t row_to_all_valu(uint32_t x, int r) {
  static_assert(ROWL == 16 || ROWL == 32, "four rows of 16 lanes or two of 32");
  if constexpr (ROWL == 16) {
    const LanePair h = swap16(x);  // [A,A,C,C] / [B,B,D,D]: one swap serves all four rows of a register, one more each pair
    x = (r & 1) ? h.b : h.a;
    r >>= 1;
  }
  const LanePair g = swap32(x);
  return r ? g.b : g.a;
}
template <int ROWL, bool VALU>
__device__ __forceinline__ uint32_t row_to_all(uint32_t x, int r) {
  if constexpr (VALU) return row_to_all_valu<ROWL>(x, r);
  return row_to_all_lds<ROWL>(x, r);
}

// ---- flat <-> tile domain ------------------------------------------------------------------
// tile-domain all-ones / zero mask (gather_mask) or 0/1 (gather) of a flat plane: tile 64s+l is bit l&31 of dword
// 2s + (l>>5) - of the wave (row 0 of a replicated PBoard plane), or of the row that starts at lane row_base (a packed one).
// One ds_bpermute and a bit-field extract: the spelling of every kernel that turns planes into per-tile records.
__device__ __forceinline__ int32_t gather_mask(uint32_t plane, int s, int row_base = 0) {
  const int lane = lane_id();
  return __builtin_amdgcn_sbfe((int32_t)bperm(((row_base + (lane >> 5)) << 2) + 8 * s, plane), (uint32_t)(lane & 31), 1u);
}
__device__ __forceinline__ uint32_t gather(uint32_t plane, int s, int row_base = 0) {
  const int lane = lane_id();
  return __builtin_amdgcn_ubfe(bperm(((row_base + (lane >> 5)) << 2) + 8 * s, plane), (uint32_t)(lane & 31), 1u);
}
// The same on the vector ALU, for the turn's own gathers (the boards' members gather / gather_mask: production, the list
// sums, army_sum), where s and row_base are wave-uniform - a slot loop's counter, a player's row: dwords 2s, 2s+1 ARE the
// 64 tiles' lane mask - two v_readlane into a scalar pair, one select.  v_readlane reads its lane whatever EXEC says: this
// spelling has no EXEC rule of its own.
__device__ __forceinline__ bool gather_flag_valu(uint32_t plane, int s, int row_base = 0) {
  const uint64_t tiles = ((uint64_t)rdlane(plane, row_base + 2 * s + 1) << 32) | (uint64_t)rdlane(plane, row_base + 2 * s);
  return __builtin_amdgcn_inverse_ballot_w64(tiles);
}
__device__ __forceinline__ int32_t gather_mask_valu(uint32_t plane, int s, int row_base = 0) { return gather_flag_valu(plane, s, row_base) ? -1 : 0; }
__device__ __forceinline__ uint32_t gather_valu(uint32_t plane, int s, int row_base = 0) { return gather_flag_valu(plane, s, row_base) ? 1u : 0u; }
template <bool VALU>
__device__ __forceinline__ int32_t gather_mask_as(uint32_t plane, int s, int row_base) {
  if constexpr (VALU) return gather_mask_valu(plane, s, row_base);
  return gather_mask(plane, s, row_base);
}
template <bool VALU>
__device__ __forceinline__ uint32_t gather_as(uint32_t plane, int s, int row_base) {
  if constexpr (VALU) return gather_valu(plane, s, row_base);
  return gather(plane, s, row_base);
}
// tile-domain predicates -> flat plane: the ballot of slot s is dwords 2s, 2s+1 of the bit string (lanes 2s, 2s+1: row 0)
__device__ __forceinline__ void ballot_to_row0(uint32_t& plane, unsigned long long ballot, int s) {
  plane = (uint32_t)gvec_llvm_writelane((int)(uint32_t)ballot, 2 * s, (int)plane);
  plane = (uint32_t)gvec_llvm_writelane((int)(uint32_t)(ballot >> 32), 2 * s + 1, (int)plane);
}

// LDS traffic inside one wave needs no s_barrier (DS ops of a wave execute in order); this
// only stops the compiler from reordering the accesses of different lanes.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// ---- the build's counter RNG (DESIGN.md "Synthetic inputs"; mirrored in oracle/) --------
__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
// env_key(lo, hi, env) = env_key_of(env_key_base(lo, hi), env): the base is a function of the launch's seed alone and
// is hashed once on the host (StepArgs::seed_base), not once per board on the scalar unit
__host__ __device__ __forceinline__ uint32_t env_key_base(uint32_t lo, uint32_t hi) { return fmix32(lo ^ 0x9E3779B9u) + hi * 0x85EBCA77u + 0x27D4EB2Fu; }
__host__ __device__ __forceinline__ uint32_t env_key_of(uint32_t base, uint32_t env) { return fmix32(base + env * 0xC2B2AE3Du); }
__host__ __device__ __forceinline__ uint32_t env_key(uint32_t lo, uint32_t hi, uint32_t env) { return env_key_of(env_key_base(lo, hi), env); }

// kColumnPattern[W] = sum of 1 << k for k = 0, W, 2W, ... < 32: where column 0 falls in a 32-tile
// window that starts in column 0
struct ColumnPatternTable {
  uint32_t v[33];
  constexpr ColumnPatternTable() : v{} {
    for (int w = 1; w <= 32; ++w) {
      uint32_t p = 0u;
      for (int k = 0; k < 32; k += w) p |= 1u << k;
      v[w] = p;
    }
  }
  __device__ __forceinline__ uint32_t operator[](int w) const { return v[w]; }
};
__device__ const ColumnPatternTable kColumnPattern{};

// ---- the header record in registers: for any board type with hv (lane k holds header dword k) and the wave-uniform
// fields W, H, P, N, turn, recipW, alive, hflags --------------------------------------------------
__device__ __forceinline__ void unpack_dims(uint32_t dims, int& W, int& H, int& P, uint32_t& hflags) {
  W = (int)(dims & 0xFFu);
  H = (int)((dims >> 8) & 0xFFu);
  P = (int)((dims >> 16) & 0xFFu);
  hflags = dims >> 24;
}
// the wave-uniform fields from the header words: word(k) is header dword k
template <typename BT, typename F>
__device__ __forceinline__ void unpack_hdr(BT& b, F&& word) {
  b.turn = (int)word(H_TURN);
  unpack_dims(word(H_DIMS), b.W, b.H, b.P, b.hflags);
  b.N = b.W * b.H;
  b.alive = word(H_STATUS) & 0xFFu;
  b.recipW = (int)word(H_RECIPW);
}
template <typename BT>
__device__ __forceinline__ void decode_hdr(BT& b) {
  unpack_hdr(b, [&](int k) { return rdlane(b.hv, k); });
}
// v must be wave-uniform (every caller passes scalar values): one v_writelane, no compare / select
template <typename BT>
__device__ __forceinline__ void hdr_set(BT& b, int k, uint32_t v) { b.hv = (uint32_t)gvec_llvm_writelane((int)v, k, (int)b.hv); }
template <typename BT>
__device__ __forceinline__ uint32_t hdr_get(const BT& b, int k) { return rdlane(b.hv, k); }
// RECIPW: H_RECIPW is written too (else it rides along in hv unchanged: a function of W); CLASS: the store's streaming
// class (st_stream; 0 = a plain store)
template <bool RECIPW, int CLASS, typename BT>
__device__ __forceinline__ void pack_hdr(BT& b, uint32_t* hdr_env, uint32_t last_err) {
  hdr_set(b, H_TURN, (uint32_t)b.turn);
  hdr_set(b, H_DIMS, (uint32_t)b.W | ((uint32_t)b.H << 8) | ((uint32_t)b.P << 16) | (b.hflags << 24));
  hdr_set(b, H_STATUS, b.alive | (last_err << 16));
  if constexpr (RECIPW) hdr_set(b, H_RECIPW, (uint32_t)b.recipW);
  if (lane_id() < HDR_DW) st_stream<CLASS>(hdr_env + lane_id(), b.hv);
}

// the player-independent half of MoveAction.Validate (core/action.go:58-64, :96-98) per direction,
// rules/legal_moves.go:13-18 order: needs the geometry masks, the type planes and W.  On PBoard: bit for bit the stored
// planes on every lane with col() < fd.  The lanes beyond hold zero in valid / ncol0 / ncolL (never loaded), so notm, ok[1]
// and ok[3] are zero there; ok[0] and ok[2] may carry the neighbouring lane's bits into column fd, where every plane they
// are ever ANDed with (own, lst, gt1: legal_planes) is zero.  Wave-uniform control flow only.
template <typename BT>
__device__ __forceinline__ void derive_targets(BT& b) {
  const uint32_t notm = ~b.mtn & b.valid;
  b.ok[0] = b.upW(notm);            // target (x, y-1)
  b.ok[1] = b.dn1(notm) & b.ncolL;  // target (x+1, y)
  b.ok[2] = b.dnW(notm);            // target (x, y+1)
  b.ok[3] = b.up1(notm) & b.ncol0;  // target (x-1, y)
}
// OwnedTiles == board ownership for every player (no owned-but-unlisted tile, H6)
template <typename BT>
__device__ __forceinline__ bool lists_match(const BT& b) {
  uint32_t d = 0u;
#pragma unroll
  for (int k = 0; k < (int)(sizeof(b.own) / sizeof(b.own[0])); ++k) d |= b.lst[k] ^ b.own[k];
  return !wave_any(d != 0u);
}
// Sets HF_LDIFF to what the lists are now: call BEFORE store_hdr; the plane stores write the list planes accordingly.
template <typename BT>
__device__ __forceinline__ void settle_lists(BT& b) {
  b.hflags = lists_match(b) ? (b.hflags & ~HF_LDIFF) : (b.hflags | HF_LDIFF);
}

// =========================================================================================
// Board: the PLAIN register layout - one register per (plane kind, player); lane i holds dword i of the bit
// string.  Used by the kernels that convert between the resident record and per-tile planes (import /
// export / records) and by the experience kernels; it owns the routines that BUILD the constant planes.
// =========================================================================================
template <int MAXP, int NSLOT>
struct Board {
  using PL = Planes<MAXP>;

  // flat domain
  uint32_t own[MAXP], lst[MAXP], vis[MAXP], chg, vch, gt1, gen, city, mtn;
  uint32_t valid;  // bits t < N
  uint32_t ncol0;  // bits with x != 0      (guards a shift towards higher t)
  uint32_t ncolL;  // bits with x != W - 1  (guards a shift towards lower t)
  uint32_t ok[4];  // the neighbour in direction d (0 up, 1 right, 2 down, 3 left) is on the board and not a mountain
  // tile domain
  int32_t army[NSLOT];
  // header: lane k holds header dword k
  uint32_t hv;
  // wave-uniform
  int W, H, P, N, turn, recipW;
  uint32_t alive, hflags;

  // ---- geometry masks of this board size (computed on import, then carried as planes) ---------
  __device__ __forceinline__ void geometry() {
    const int t0 = 32 * (lane_id() & 31);
    const int left = N - t0;
    valid = (lane_id() >= 32 || left <= 0) ? 0u : (left >= 32 ? 0xFFFFFFFFu : ((1u << left) - 1u));
    const uint32_t pat = kColumnPattern[W];  // bits at multiples of W below 32 (one scalar load)
    // 24-bit multiplies are full rate (v_mul_lo_u32 is quarter rate); t0 < 2048, recipW <= 65536, W <= 32
    const int q = (int)(__umul24((uint32_t)t0, (uint32_t)recipW) >> 16);  // t0 / W, exact for t0 < 1024
    const int x0 = t0 - (int)__umul24((uint32_t)q, (uint32_t)W);          // column of this lane's first tile
    const uint32_t col0 = pat << (x0 ? W - x0 : 0);
    ncol0 = ~col0;
    ncolL = ~__builtin_amdgcn_alignbit(from_next(col0), col0, 1);  // t is in the last column iff t+1 is in column 0
    ncol0 = (lane_id() < 32) ? ncol0 : 0xFFFFFFFFu;                // lanes beyond the bit string hold no tiles: any value
    ncolL = (lane_id() < 32) ? ncolL : 0xFFFFFFFFu;                // would do, a fixed one keeps the stored planes canonical
  }
  // the header flags that are functions of the board, and "nothing is known" for the turn engine's bookkeeping
  // flags: wherever a board is imported or modified from outside
  __device__ __forceinline__ void static_flags() {
    const int special = (int)wave_sum((uint32_t)__builtin_popcount(gen | city));
    hflags = (hflags & ~(HF_SYNC | HF_VSMALL | HF_FEWSPECIAL)) | ((2 * P + special <= N / 5) ? HF_FEWSPECIAL : 0u);
  }
  // Tile.Army > 1 as a flat plane
  __device__ __forceinline__ void refresh_gt1() {
    gt1 = 0u;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) ballot_to_row0(gt1, __builtin_amdgcn_ballot_w64(army[s] > 1), s);
  }

  // ---- flat-string shifts: bit t of the result = bit (t -+ k) of m ---------------------------
  __device__ __forceinline__ uint32_t up1(uint32_t m) const { return __builtin_amdgcn_alignbit(m, from_prev(m), 31); }  // from t-1
  __device__ __forceinline__ uint32_t dn1(uint32_t m) const { return __builtin_amdgcn_alignbit(from_next(m), m, 1); }   // from t+1
  __device__ __forceinline__ uint32_t upW(uint32_t m) const {                                                           // from t-W
    return __builtin_amdgcn_alignbit(m, from_prev(m), (uint32_t)(32 - W) & 31u);
  }
  __device__ __forceinline__ uint32_t dnW(uint32_t m) const {  // from t+W
    return (uint32_t)((((uint64_t)from_next(m) << 32) | (uint64_t)m) >> W);
  }

  // ---- load / store ---------------------------------------------------------------------
  __device__ __forceinline__ void load_hdr(const uint32_t* hdr_env) {
    const int lane = lane_id();
    hv = (lane < HDR_DW) ? hdr_env[lane] : 0u;
    decode_hdr(*this);
  }
  __device__ __forceinline__ void store_hdr(uint32_t* hdr_env, uint32_t last_err) { pack_hdr<true, 0>(*this, hdr_env, last_err); }

  __device__ __forceinline__ void load_planes(const uint32_t* rows_env, int fd) {
    const int lane = lane_id();
    const bool on = lane < fd;
    const uint32_t* g = rows_env + (on ? lane : 0);
    auto ld = [&](int plane) {
      const uint32_t v = g[plane * fd];
      return on ? v : 0u;
    };
    const bool listed = (hflags & HF_LDIFF) != 0u;  // needs the header: call after load_hdr
#pragma unroll
    for (int p = 0; p < MAXP; ++p) {
      own[p] = ld(PL::OWN + p);
      vis[p] = ld(PL::VIS + p);
      lst[p] = own[p];
      if (listed) lst[p] = ld(PL::LST + p);
    }
    chg = ld(PL::CHG);
    vch = ld(PL::VCH);
    gt1 = ld(PL::GT1);
    gen = ld(PL::GEN);
    city = ld(PL::CITY);
    mtn = ld(PL::MTN);
    valid = ld(PL::VALID);
    ncol0 = ld(PL::NCOL0);
    ncolL = ld(PL::NCOLL);
#pragma unroll
    for (int d = 0; d < 4; ++d) ok[d] = ld(PL::OK + d);
  }

  // The planes from GEN on change only when a board is imported or re-dealt (with_types).  all_lists: write the list
  // planes whatever the flag says (a record slab is complete on its own).
  __device__ __forceinline__ void store_planes(uint32_t* rows_env, int fd, int row_dw, bool with_types, bool all_lists = false) const {
    const int lane = lane_id();
    if (lane < fd) {
      uint32_t* g = rows_env + lane;
#pragma unroll
      for (int p = 0; p < MAXP; ++p) {
        g[(PL::OWN + p) * fd] = own[p];
        g[(PL::VIS + p) * fd] = vis[p];
        if (all_lists || (hflags & HF_LDIFF)) g[(PL::LST + p) * fd] = lst[p];
      }
      g[PL::CHG * fd] = chg;
      g[PL::VCH * fd] = vch;
      g[PL::GT1 * fd] = gt1;
      if (with_types) {
        g[PL::GEN * fd] = gen;
        g[PL::CITY * fd] = city;
        g[PL::MTN * fd] = mtn;
        g[PL::VALID * fd] = valid;
        g[PL::NCOL0 * fd] = ncol0;
        g[PL::NCOLL * fd] = ncolL;
#pragma unroll
        for (int d = 0; d < 4; ++d) g[(PL::OK + d) * fd] = ok[d];
      }
    }
    if (with_types && lane < row_dw - PL::COUNT * fd) rows_env[PL::COUNT * fd + lane] = 0u;  // the block's padding
  }

  // ---- internal/experience/rewards.go helpers ---------------------------------------------------
  // sum of Tile.Army over a flat plane (countPlayerArmies, rewards.go:98-107)
  static __device__ __forceinline__ int32_t gather_mask(uint32_t plane, int s) { return gather_mask_as<(GVEC_XLANE & GVEC_XL_GATHER) != 0>(plane, s, 0); }
  __device__ __forceinline__ int32_t army_sum(uint32_t plane) const {
    int32_t acc = 0;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) acc += army[s] & gather_mask(plane, s);
    return (int32_t)wave_sum((uint32_t)acc);
  }
  __device__ __forceinline__ int32_t count(uint32_t plane) const { return (int32_t)wave_sum((uint32_t)__builtin_popcount(plane)); }
};

}  // namespace gvec
