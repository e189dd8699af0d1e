/*
 * generals_vec.h — C ABI of the MI355X-native batched Generals.io turn engine.
 *
 * This is the drop-in boundary for ONE hot path of
 * mitchelldurbincs/GeneralsReinforcementLearning: the per-game turn loop of
 * internal/game + internal/game/core (movement/combat, production, 3x3 fog of
 * war, legal-action mask), batched over B independent boards ("envs").
 *
 * The reference has no FFI seam; the seam is the Go method set of *game.Engine
 * (internal/game/engine.go:62-298).  Every entry point below names the Go
 * symbol(s) it replaces.  A cgo shim binds these 1:1.
 *
 * Conventions
 *   - All functions return int32 status: 0 = GVEC_OK, negative = API misuse /
 *     runtime failure (never a game-rule error).  Per-env game-rule errors are
 *     delivered in int32 err[B] using the sentinel numbering of
 *     internal/game/core/errors.go:8-17 == proto/common/v1/common.proto:39-48.
 *   - Buffers are caller-owned, env-major.  `mem` says where they live:
 *     GVEC_MEM_HOST (the library copies through its own device staging buffers) or
 *     GVEC_MEM_DEVICE (pointers are HIP device pointers on the handle's device;
 *     no host copy, work is enqueued on the handle's stream and NOT synchronised).
 *   - Tile planes use the reference's row-major index  t = y*W + x
 *     (core/board.go:108) with the env's OWN width W, packed at the start of a
 *     slot of max_width*max_height elements (padded batch, SURVEY config 5).
 *   - A handle is not thread-safe (mirrors Engine: externally serialised,
 *     internal/grpc/gameserver/game_manager.go:576-602).
 *   - A handle lives on ONE device (gvec_create) or spans several (gvec_create_sharded).
 *   - There is NO CPU fallback behind this ABI: every compute entry point runs
 *     hand-written HIP kernels for gfx950 and fails with GVEC_E_NO_DEVICE when no
 *     GPU is present.
 */
#ifndef GENERALS_VEC_H
#define GENERALS_VEC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GVEC_ABI_VERSION 2

/* limits of this build */
#define GVEC_MAX_PLAYERS 8   /* VisibleBitfield is carried as a u8 per tile            */
#define GVEC_MAX_DIM     32  /* one board row is one u32 bit-row on the device          */

/* API status (negative) */
#define GVEC_OK            0
#define GVEC_E_INVALID    -1  /* bad argument                                           */
#define GVEC_E_NO_DEVICE  -2  /* no HIP device / device init failed                     */
#define GVEC_E_HIP        -3  /* HIP runtime error (see gvec_last_error)                */
#define GVEC_E_RANGE      -4  /* env range / size out of bounds                         */
#define GVEC_E_BOARD      -5  /* reset/write_state input violates the board contract    */

/* per-env game errors (core/errors.go:8-17; common.proto:39-48) */
#define GVEC_ERR_NONE                 0
#define GVEC_ERR_INVALID_COORDINATES  1
#define GVEC_ERR_NOT_ADJACENT         2
#define GVEC_ERR_NOT_OWNED            3
#define GVEC_ERR_INSUFFICIENT_ARMY    4
#define GVEC_ERR_GAME_OVER            5
#define GVEC_ERR_INVALID_PLAYER       6
#define GVEC_ERR_MOVE_TO_SELF         7
#define GVEC_ERR_TARGET_IS_MOUNTAIN   8

/* tile types (core/board.go:20-26) */
#define GVEC_TILE_NORMAL   0
#define GVEC_TILE_GENERAL  1
#define GVEC_TILE_CITY     2
#define GVEC_TILE_MOUNTAIN 3
#define GVEC_NEUTRAL      (-1)

#define GVEC_MEM_HOST   0
#define GVEC_MEM_DEVICE 1

/* One player's action for one turn == *core.MoveAction (core/action.go:23-36)
 * after convertProtoAction (internal/grpc/gameserver/converters.go:105-132).
 * Coordinates are clamped Go ints: any out-of-board value stays out of board,
 * so MoveAction.Validate's ErrInvalidCoordinates branch is preserved.
 * The slot index in actions[env][player] is MoveAction.PlayerID. */
#define GVEC_ACT_VALID 1u   /* 0 = nil action (no-op this turn)                        */
#define GVEC_ACT_HALF  2u   /* proto Action.half; MoveAll = !half                      */
#define GVEC_ACT_SKIP_ENV 4u /* on actions[env][0] only: this env does not play a turn in
                               this call (err 0, state untouched).  Lets a vector env
                               mirror clients whose games advance at different times
                               (python/generals_gym/generals_env.py:226-241 returns
                               before submitting anything on an invalid action).         */
#define GVEC_ACT_RESET_ENV 8u /* on actions[env][0] only, handles with auto_reset and a board pool: this env
                                is re-dealt from the pool in this call whether or not its game is over
                                (err 0) - how a vector env ends a truncated episode
                                (generals_env.py:283-284: truncated = turn_count >= max_turns) without
                                reading `done` back and poking it.  Ignored without a pool.          */
typedef struct gvec_action {
  int8_t  from_x, from_y, to_x, to_y;
  uint8_t flags;
  uint8_t reserved[3];
} gvec_action; /* 8 bytes */

typedef struct gvec_config {
  int32_t abi_version;            /* GVEC_ABI_VERSION                                    */
  int32_t num_envs;               /* B                                                   */
  int32_t max_width, max_height;  /* <= GVEC_MAX_DIM each                                */
  int32_t max_players;            /* <= GVEC_MAX_PLAYERS                                 */
  int32_t device;                 /* HIP device ordinal                                  */
  int32_t fog_of_war;             /* GameState.FogOfWarEnabled (engine_initializer.go:118 = 1) */
  int32_t prod_general;           /* config.go:206  game.production.general = 1          */
  int32_t prod_city;              /* config.go:207  = 1                                  */
  int32_t prod_normal;            /* config.go:208  = 1                                  */
  int32_t normal_growth_interval; /* config.go:209  = 25                                 */
  int32_t auto_reset;             /* 1: a finished env is re-dealt from the board pool on
                                     its next step (vector-env semantics; no Go analogue) */
  int32_t reserved[4];
} gvec_config;

typedef struct gvec_handle gvec_handle;

/* Optional-plane view used by gvec_read_state / gvec_write_state.  NULL = skip.
 * Shapes: tile planes [n][max_width*max_height]; per-player [n][max_players];
 * scalars [n]. */
typedef struct gvec_state_view {
  int32_t* army;         /* Tile.Army (core/board.go:9).  A Go int is 64-bit; this engine computes in
                            int32 and stores exactly (u16 or int32 per env): a board whose armies
                            pass 2^31-1 would wrap here and not in Go - unreachable by play
                            (production adds 1 per tile per turn), reachable by gvec_write_state */
  int8_t*  owner;        /* Tile.Owner, -1 neutral         (core/board.go:8)            */
  uint8_t* type;         /* Tile.Type                      (core/board.go:10)           */
  uint8_t* visible;      /* Tile.VisibleBitfield, bit p    (core/board.go:11)           */
  int8_t*  listed;       /* p iff t in Players[p].OwnedTiles, else -1 (game/state.go:12)*/
  uint8_t* changed;      /* 1 iff t in GameState.ChangedTiles          (state.go:29)    */
  uint8_t* vis_changed;  /* 1 iff t in GameState.VisibilityChangedTiles (state.go:33)   */
  int32_t* turn;         /* GameState.Turn                                              */
  uint8_t* done;         /* Engine.gameOver                 (engine.go:20)              */
  int8_t*  winner;       /* Engine.GetWinner()              (engine.go:248-263)         */
  int32_t* width;        /* Board.W                                                     */
  int32_t* height;       /* Board.H                                                     */
  int32_t* players;      /* len(GameState.Players)                                      */
  uint8_t* alive;        /* Player.Alive                    (state.go:9)                */
  int32_t* army_count;   /* Player.ArmyCount                (state.go:10)               */
  int32_t* tile_count;   /* len(Player.OwnedTiles)                                      */
  int32_t* general_idx;  /* Player.GeneralIdx (highest listed general tile, -1 if none) */
} gvec_state_view;

typedef struct gvec_rollout_stats {
  int64_t env_steps;     /* turns actually advanced (live envs x turns)                 */
  int64_t aborted_turns; /* turns that returned a move-validation error     */
  int64_t games_finished;
  int64_t reserved;      /* always 0 (keeps the struct at 32 bytes)                        */
} gvec_rollout_stats;

/* ---- lifecycle ---------------------------------------------------------------- */

int32_t gvec_abi_version(void);
/* Fills the reference defaults (config.go:206-209, engine_initializer.go:118). */
int32_t gvec_config_default(gvec_config* cfg);
/* Replaces game.NewEngine for B engines (engine.go:62-71); boards arrive via gvec_reset. */
int32_t gvec_create(const gvec_config* cfg, gvec_handle** out);
int32_t gvec_destroy(gvec_handle* h);
/* One handle over several GPUs ("device list ... one handle may span several GPUs").  The B = cfg->num_envs
 * boards are split into num_devices contiguous shards whose sizes differ by at most one (shard i: base + (i < rem) envs
 * from i*base + min(i, rem), base = B / n, rem = B % n); shard i lives on devices[i] for the whole run (cfg->device is
 * ignored; a device may be listed more than once).  Boards are independent: no call moves board state between devices.
 * Every entry point that takes GVEC_MEM_HOST buffers works on the sharded handle exactly as on a plain one - the
 * caller's arrays are env-major over all B envs, every shard serves its slice, all devices at once - and the batch plays
 * the same games whatever the number of shards (a shard's agent / auto-reset / map-generator draws are keyed by the
 * env's index in the BATCH).  Entry points that take device pointers (GVEC_MEM_DEVICE, gvec_gym_*, gvec_export/import_
 * records, gvec_device_buffer, gvec_set_stream, gvec_experience_records) act on one device: use them on the child handle
 * gvec_shard returns (valid until the sharded handle is destroyed; never destroy it yourself).  Still not thread-safe:
 * one caller at a time per sharded handle (internally one worker thread per shard). */
int32_t gvec_create_sharded(const gvec_config* cfg, const int32_t* devices, int32_t num_devices, gvec_handle** out);
int32_t gvec_num_shards(const gvec_handle* h);   /* 0 for a plain handle */
int32_t gvec_shard(gvec_handle* h, int32_t i, gvec_handle** child, int32_t* env_begin, int32_t* num_envs, int32_t* device);
/* The one exchange step of the path on a sharded handle: every shard writes the compact experience records
 * (gvec_experience_records: needs gvec_experience_begin[_range] before the step) of ITS envs
 * [shard_env_begin, shard_env_begin + n) - indices inside the shard, the same slice on every device - and ships them to one
 * place: dst receives num_shards * n records, shard i's at record i * n; a record's env id is env_id_base + the env's
 * index in the batch.  mem = GVEC_MEM_HOST: dst is host memory, each device copies its slab straight to it over its own
 * PCIe link (what the Go StreamAggregator side, internal/grpc/gameserver/stream_aggregator.go:75-155, consumes);
 * mem = GVEC_MEM_DEVICE: dst is device memory on dst_device, the slabs travel GPU-to-GPU (hipMemcpyPeerAsync: xGMI on an
 * MI355X node) - for a learner that lives on a GPU.  Returns when every slab has landed. */
int32_t gvec_gather_experience_records(gvec_handle* h, int32_t shard_env_begin, int32_t n, int32_t env_id_base, int32_t mem,
                                       int32_t dst_device, void* dst);
/* Work is enqueued on this hipStream_t (default: the null stream). */
int32_t gvec_set_stream(gvec_handle* h, void* hip_stream);
int32_t gvec_synchronize(gvec_handle* h);
const char* gvec_last_error(void);

/* Page-locked host memory for the GVEC_MEM_HOST entry points: buffers obtained here are copied to / from the device at full
 * PCIe rate (a pageable buffer - a Go slice, a numpy array - goes through the driver's bounce buffers at a fraction of
 * it: 218 MB of legal masks per step at 262,144 boards take 18 ms pageable, 4 ms pinned).  Any host pointer is accepted by
 * every entry point; these are simply faster.  A cgo host passes them as unsafe.Pointer / slices over C memory. */
int32_t gvec_host_alloc(uint64_t bytes, void** out);
int32_t gvec_host_free(void* p);

/* sizes */
int32_t gvec_num_envs(const gvec_handle* h);
int32_t gvec_tile_stride(const gvec_handle* h);   /* max_width*max_height              */
int32_t gvec_mask_bytes(const gvec_handle* h);    /* bytes of one player's packed mask: 4 direction bit-planes (see gvec_step) */
int64_t gvec_state_bytes_per_env(const gvec_handle* h); /* bytes of one env's state record (gvec_export_records) */

/* ---- reset: EngineInitializer.Initialize minus mapgen -------------------------
 * (engine_initializer.go:113-143,218-225): upload boards, Turn=0, then the a15
 * pass: full stats (stats.go:33-63), full fog (visibility_optimized.go:33-53) if
 * fog_of_war, game-over check (engine.go:160-194).
 * env_ids NULL => envs 0..n-1.  owner must be in [-1, P). */
int32_t gvec_reset(gvec_handle* h, const int32_t* env_ids, int32_t n,
                   const int32_t* army, const int8_t* owner, const uint8_t* type,
                   const int32_t* width, const int32_t* height, const int32_t* players,
                   int32_t mem);

/* Deterministic on-device map generator with the algorithm and ratios of
 * internal/game/mapgen/generator.go:25-253 (Go math/rand is not reproducible
 * here: boards are keyed by (seed, env) through the library's own counter RNG).
 * Generates a board for every env (sizes per env: width/height/players arrays
 * [B] on host, or NULL = max sizes) and runs the reset pass. */
int32_t gvec_reset_generated(gvec_handle* h, uint64_t seed,
                             const int32_t* width, const int32_t* height,
                             const int32_t* players);
/* The same generator on Go's OWN math/rand: env i gets exactly the board
 *     mapgen.NewGenerator(mapgen.DefaultMapConfig(W, H, P), rand.New(rand.NewSource(seeds[i]))).GenerateMap()
 * builds (mapgen/generator.go:56-75) - i.e. the board game.NewEngine(ctx, GameConfig{Width, Height, Players, Rng:
 * rand.New(rand.NewSource(seeds[i]))}) starts from (engine_initializer.go:106-110) - then the reset pass.  Go's generator
 * (go 1.24: an additive lagged Fibonacci generator seeded through an LCG and a 607-word table) is restated from its
 * published algorithm, the table derived (scripts/gen_go_rand_cooked.py), and the whole pinned by the reference's own
 * seed-12345 tests (mapgen/generator_test.go:61-85, :396-455) through the oracle twin.  seeds: host int64 [B]; sizes as
 * gvec_reset_generated.  A Go host can therefore build B reference engines from seeds and this handle from the same seeds
 * and compare them from turn 0 (host/go/vecengine_diff_test.go). */
int32_t gvec_reset_go_seeded(gvec_handle* h, const int64_t* seeds, const int32_t* width, const int32_t* height,
                             const int32_t* players);
/* Pool of pre-generated, pre-initialised boards used by auto_reset: board j is
 * generated with key (seed, j) and sizes width[j]/height[j]/players[j] (host arrays
 * [pool_size], NULL = max sizes).  A finished env spends its next step being
 * re-dealt board mulhi(fmix32(env_key(seed, env) ^ episode*0x9E3779B1), pool_size). */
int32_t gvec_build_board_pool(gvec_handle* h, int32_t pool_size, uint64_t seed,
                              const int32_t* width, const int32_t* height,
                              const int32_t* players);

/* ---- the hot path ---------------------------------------------------------------
 * Engine.Step for every env (engine.go:75 -> turn_processor.go:29-77):
 * actions[B][max_players]; err[B] receives the sentinel of the first failing move
 * in PlayerID order (processor/action_processor.go:36-99), GVEC_ERR_GAME_OVER for
 * a finished env (turn_processor.go:95-113), else 0.
 * legal_bits (may be NULL): [B][max_players][mask_bytes], computed on the post-step
 * state.  One player's mask is FOUR DIRECTION BIT-PLANES of mask_bytes/4 bytes each,
 * d = 0 up, 1 right, 2 down, 3 left (rules/legal_moves.go:13-18,66): bit t (LSB
 * first) of plane d = Engine.GetLegalActionMask(p)[t*4 + d], t = y*W + x.  (Go's
 * []bool index order is a transpose of this: see INTEGRATION.md for the 3-line
 * unpack.)  ABI version 2: version 1 packed bit i = mask[i].
 * Alignment with GVEC_MEM_DEVICE: none beyond the types'.  The kernel writes the masks into the handle's own resident
 * buffer (16-byte aligned; gvec_device_buffer) and legal_bits receives a device-to-device copy of it, so a byte array
 * may sit at any address; the same holds for gvec_legal_mask. */
int32_t gvec_step(gvec_handle* h, const gvec_action* actions, int32_t* err,
                  uint8_t* legal_bits, int32_t mem);

/* Engine.GetLegalActionMask for all envs/players (engine.go:271-280). */
int32_t gvec_legal_mask(gvec_handle* h, uint8_t* legal_bits, int32_t mem);

/* Engine.ComputePlayerVisibility(player) for all envs
 * (visibility_optimized.go:166-195): visible/fog are [B][tile_stride] 0/1 bytes;
 * either may be NULL. */
int32_t gvec_player_visibility(gvec_handle* h, int32_t player,
                               uint8_t* visible, uint8_t* fog, int32_t mem);

/* Engine.GameState() / IsGameOver / GetWinner / GetChangedTiles /
 * GetVisibilityChangedTiles (engine.go:197-198,248-298) for envs
 * [env_begin, env_begin+n). */
int32_t gvec_read_state(gvec_handle* h, int32_t env_begin, int32_t n,
                        const gvec_state_view* view, int32_t mem);
/* Raw poke of engine state (what the reference's tests do by writing e.gs.*
 * directly, e.g. action_mask_test.go:62-68); no init pass is run. Planes that are
 * NULL keep their current contents. */
int32_t gvec_write_state(gvec_handle* h, int32_t env_begin, int32_t n,
                         const gvec_state_view* view, int32_t mem);

/* ---- synthetic random-agent rollouts (BASELINE.json metric) ---------------------
 * K turns for every env with the on-device random agent of SURVEY 8(d): per alive
 * player uniform choice over Engine.GetLegalActionMask, half with p=0.3, no-op
 * with p=0.1, `invalid_permille`/1000 deliberately unchecked moves (H5 stress);
 * counter RNG keyed by (seed, env, turn, player).  fused != 0 keeps board state in
 * registers/LDS across the K turns of one launch; fused == 0 issues one step launch
 * per turn (same results).  stats may be NULL. */
int32_t gvec_rollout(gvec_handle* h, int32_t turns, uint64_t seed,
                     int32_t invalid_permille, int32_t fused,
                     gvec_rollout_stats* stats);
/* The per-turn rollout (fused = 0, no statistics) for envs [env_begin, env_begin + n) only: the same launch over a slice
 * of the batch.  Disjoint slices may be stepped on different streams (gvec_set_stream before each call) and overlap on the
 * GPU - how a consumer steps a sampled slice together with its snapshot / record kernels beside the rest of the batch
 * (bench.py's gathering steps).  Stepping every env exactly once, slice by slice, equals one gvec_rollout turn. */
int32_t gvec_rollout_range(gvec_handle* h, int32_t env_begin, int32_t n, int32_t turns, uint64_t seed, int32_t invalid_permille);
/* The agent's mix: a player sits a turn out when (draw & 0xFFFF) < noop_per_65536 (default 6554,
 * p = 0.1) and moves half its army when (draw >> 16) < half_per_65536 (default 19661, p = 0.3).
 * (45875, 19661) are the rates of the reference's game.GenerateRandomActions (demo_helpers.go:20,44:
 * a player acts with p = 0.3, MoveAll with p = 0.7); (0, 0) always plays a full move, uniform over
 * the legal ones.  The default acts three times as often as the Go helper: more work per turn.
 * Applies to gvec_rollout and gvec_agent_actions. */
int32_t gvec_set_agent_mix(gvec_handle* h, int32_t noop_per_65536, int32_t half_per_65536);
/* Lifetime counters summed over every env of the handle (absolute values; gvec_rollout's stats are the
 * difference of two such reads): env_steps = engine turns actually PLAYED - a step that re-deals a finished
 * env, a frozen env or a GVEC_ACT_SKIP_ENV env plays none -, aborted_turns, games_finished.
 * One small reduction launch + an 24-byte read-back; synchronises the handle's stream. */
int32_t gvec_counters(gvec_handle* h, gvec_rollout_stats* out);
/* The HBM bytes ONE env-step of the hot path (gvec_step / per-turn gvec_rollout) must move BY CONSTRUCTION of the
 * resident layout, from the same constants the kernel is compiled with:
 * out4[0] read  = header + the mutable and constant planes the step kernel fetches (not the move-target planes where it
 *                 rebuilds them) + narrow armies (less an odd last slot's dead half)
 * out4[1] write = header + mutable planes (rounded up to a whole 16-byte chunk) + narrow armies
 * out4[2] mask  = the legal masks written when legal_bits / the agent is on (max_players * mask_bytes)
 * out4[3] extra = what an env in the rare forms adds on top (list planes both ways + the int32 army escape both ways)
 * bench.py prices roofline.frac with read + write + mask. */
int32_t gvec_step_traffic_bytes(const gvec_handle* h, int64_t* out4);
/* The agent alone: fills actions[B][max_players] for the current state/turn. */
int32_t gvec_agent_actions(gvec_handle* h, uint64_t seed, int32_t invalid_permille,
                           gvec_action* actions, int32_t mem);
/* Scripted opponent: for every env, the move of each player whose bit is set in `players` (bits below max_players),
 * written into actions[B][max_players]; the other slots are left untouched (host memory included).  The rule (DESIGN.md
 * section 6 "Scripted opponent") reads the player's own view only - what fog lets it see - and plays MoveAll: the best
 * capture by target tier (enemy general > city > enemy tile > neutral tile), then margin, else one step of the largest
 * army towards the nearest target.  A slot plays gvec_agent_actions(seed, 0)'s move instead (under the current
 * gvec_set_agent_mix) with probability random_permille / 1000, drawn per (seed, env, turn, player); 0 = the pure rule,
 * 1000 = the random agent.  random_permille outside [0, 1000] or a bit at or above max_players: GVEC_E_INVALID.
 * Sharded handles: host memory only. */
int32_t gvec_bot_actions(gvec_handle* h, uint32_t players, uint64_t seed, int32_t random_permille,
                         gvec_action* actions, int32_t mem);

/* ---- flat Monte Carlo search: what happens if this seat plays move a here? ------------
 * For every root i < num_roots, candidate k < num_candidates and replica j < replicas, playout v = (i*K + k)*R + j starts
 * from the state of env root_envs[i] (NULL: env i), plays candidates[i][k] for seat root_players[i] on its first turn while
 * every other alive seat plays the on-device random agent, then up to depth - 1 further turns with the agent on every seat,
 * and writes terms[v][GVEC_SEARCH_TERMS]:
 *   0 valid        the row was played (an invalid row is all zeros)
 *   1 turns        turns played, <= depth: a finished game ends its playout (never re-dealt, whatever auto_reset says)
 *   2 alive        the seat is alive at the end
 *   3 won          the game is over and the seat is Engine.GetWinner
 *   4 land, 5 army the seat's tile_count and ArmyCount at the end
 *   6 land_others, 7 army_others   the sums over the other seats
 * A candidate is a gym action index, tile*5 + {up, right, down, left, half}, decoded against the seat's own valid-action
 * mask exactly as gvec_gym_step_players decodes a learner's action, or GVEC_SEARCH_PASS: the seat plays no move on its
 * first turn.  A row is invalid when the candidate is anything else that the decode does not accept (GVEC_SEARCH_NONE, the
 * padding value, among them), when the root env is outside [0, num_envs) (checked on the device), when the root game is
 * over, or when the seat is not alive (which covers a seat at or above the env's player count).
 * The agent's draws are keyed by (seed, PLAYOUT index v, turn, player) under the handle's current gvec_set_agent_mix, with
 * no unchecked moves: the call equals gvec_copy_envs of the roots, each repeated K*R times, into a scratch handle of n*K*R
 * envs without a board pool, one gvec_step with gvec_agent_actions(seed, 0)'s moves in which the seat's slot is replaced
 * by the candidate, gvec_rollout(depth - 1, seed, 0, fused) and the eight numbers read from gvec_read_state - bit for bit,
 * in one launch that writes 32 bytes per playout and nothing else.  The roots are read only: their headers (lifetime
 * counters included), planes, armies, the legal-mask buffer, the per-env error codes and the recorded actions keep every
 * byte.  The playouts see the true state, not the seat's fogged view.
 * Every pointer is device memory.  Enqueued on the handle's stream; nothing is synchronised.  num_roots == 0: nothing to do.
 * GVEC_E_INVALID with a gvec_last_error message naming the field: args, root_players, candidates, terms or h NULL, a negative
 * num_roots, num_candidates / replicas / depth below 1, n*K*R at or above 2^31.  Sharded handles: call it on gvec_shard. */
#define GVEC_SEARCH_TERMS 8
#define GVEC_SEARCH_PASS  (-1)
#define GVEC_SEARCH_NONE  (-2)
typedef struct gvec_search_args {
  int32_t num_roots, num_candidates, replicas, depth;   /* n, K, R, D >= 1 */
  const int32_t* root_envs;     /* device [n], NULL = 0..n-1 */
  const int32_t* root_players;  /* device [n] */
  const int64_t* candidates;    /* device [n][K] */
  uint64_t seed;
  int32_t* terms;               /* device [n][K][R][GVEC_SEARCH_TERMS] */
} gvec_search_args;
int32_t gvec_search_playouts(gvec_handle* h, const gvec_search_args* args);
/* The same search with playouts that play the game: in every playout turn the seats whose bit is set in bot_players (an
 * absolute seat mask, gvec_bot_actions' `players`) play the scripted opponent's rule instead of the random agent's draw -
 * each with probability bot_random_permille / 1000 the agent's draw after all, as gvec_bot_actions mixes it.  The searched
 * seat's candidate still replaces its slot on the first turn, whether the seat is on the rule or not.  The call equals
 * gvec_copy_envs of the roots into a scratch handle of n*K*R envs and then, per turn, gvec_agent_actions(seed, 0),
 * gvec_bot_actions(bot_players, seed, bot_random_permille) over its result, the candidate on the first turn, gvec_step -
 * bit for bit, in one launch: env v of the scratch handle draws what playout v draws, for the agent and for the mix.
 * bot_players == 0 gives gvec_search_playouts' terms.  Everything else - args, terms, invalid rows, read-only roots - is as
 * above.  GVEC_E_INVALID, besides the cases above: bot_random_permille outside [0, 1000], a bit of bot_players at or above
 * max_players. */
int32_t gvec_search_playouts_bot(gvec_handle* h, const gvec_search_args* args, uint32_t bot_players, int32_t bot_random_permille);

/* ---- sequential-halving search: what lies between two playout launches, and the policy target ----
 * The root search of Danihelka et al., "Policy improvement by planning with Gumbel" (ICLR 2022): m candidates per row, drawn
 * by the caller, are played in rounds; every round's playouts (gvec_search_playouts' terms) are added to a running sum and
 * count per initial candidate SLOT, and the better part of the round's columns goes on to the next one.  Both entry points
 * are handle-free: (device, hip_stream, args), every pointer device memory, enqueued on hip_stream, nothing synchronised.
 * One wavefront per row.
 *
 * gvec_search_halve, once per round.  This round played k columns of `replicas` playouts per row; column c < k stands for
 * the initial slot s = slot[r][c] (slot NULL: s = c, which needs k == m).  The slots of a row are distinct and in [0, m); a
 * column whose slot is not is left out altogether.  Per row:
 *   1. for j = 0 .. replicas - 1 in that order, a playout terms[r][c][j] whose `valid` term is non-zero adds its score to
 *      sum[r][s] and 1 to count[r][s].  The score, in float64 and in this order of operations: `win` if the won term is
 *      non-zero, else `loss` if the alive term is zero, else
 *        (land * ratio(t.land, t.land_others) + army * ratio(t.army, t.army_others)) - (land + army) / 2,
 *      ratio(a, b) = a / (a + b), or 0.5 when a + b == 0.  Slots that no column names keep their sum and count.
 *   2. nmax = the largest count over the row's m slots after step 1.  A slot with count > 0 has mean = sum / count and
 *        key = prior_key[r][s] + ((c_visit + nmax) * c_scale) * ((mean - q_lo) * q_inv_range)       (float64, this grouping)
 *      The caller passes q_lo = min(loss, -(land + army) / 2) and q_inv_range = 1 / (max(win, (land + army) / 2) - q_lo):
 *      the playout value on [0, 1].
 *   3. the k columns are ranked: a LIVE column (count > 0 and candidates0[r][s] != GVEC_SEARCH_NONE) before one that is
 *      not; among live columns the larger key, then the lower slot; among the others the lower slot.  The column of rank
 *      q < k_next writes next_slot[r][q] = s and next_candidates[r][q] = candidates0[r][s]: a row with fewer than k_next
 *      live columns carries its padding on, and the playout kernel answers it with invalid rows again.
 * sum float64 [n][m] and count int32 [n][m] are read and written (the caller zeroes them before the first round);
 * next_slot int32 [n][k_next] and next_candidates int64 [n][k_next] are written.  No atomics: a row belongs to one
 * wavefront and a slot to one lane, so the same input gives the same bits.
 * GVEC_E_INVALID (with a gvec_last_error message) before anything touches a device: args or a pointer other than slot
 * NULL, n < 0, m outside [1, 64], k outside [1, m], k_next outside [1, k], replicas < 1, slot NULL with k != m.  n == 0 is a
 * no-op that needs no device.
 *
 * gvec_search_improved_policy: the policy target from completed Q values over ALL legal actions.  Per row, with S = {i :
 * mask_i != 0} and x_i = logits_i (0 when logits is NULL: the uniform prior), pi = softmax_S(x):
 *   V      the slots with count > 0 whose candidate a lies in [0, num_actions) and in S (a visited GVEC_SEARCH_PASS has no
 *          action index and is left out); q(a) = sum / count, N = the sum of count over V, nmax = the largest count of the
 *          row's m slots
 *   v_mix  (value + N * vq) / (1 + N) with vq = sum_V pi(a) q(a) / sum_V pi(a); value NULL: v_mix = vq.  V empty: v_mix =
 *          value, or 0 without one
 *   target softmax_S(x_i + ((c_visit + nmax) * c_scale) * ((q_i - q_lo) * q_inv_range)), q_i = q(a) on V and v_mix elsewhere;
 *          0 outside S; all zeros for a row with S empty; softmax_S(x) itself when V is empty
 * target float32 [n][num_actions]: EVERY element is written; v_mix float32 [n].  float32 arithmetic with fixed reduction
 * orders (q(a) is the float64 quotient rounded once); the row is read from HBM once and held in registers.
 * GVEC_E_INVALID before anything touches a device: args, mask, candidates0, sum, count, target or v_mix NULL, n < 0,
 * num_actions outside [1, 5 * GVEC_MAX_DIM * GVEC_MAX_DIM], m outside [1, 64].  n == 0 is a no-op that needs no device. */
#define GVEC_SEARCH_MAX_SLOTS 64
typedef struct gvec_search_halve_args {
  int32_t n, m, k, replicas, k_next, reserved;
  const int32_t* terms;             /* [n][k][replicas][GVEC_SEARCH_TERMS] */
  const int32_t* slot;              /* [n][k], NULL = identity */
  const int64_t* candidates0;       /* [n][m] */
  const double* prior_key;          /* [n][m] */
  double win, loss, land, army;     /* the score's weights */
  double q_lo, q_inv_range, c_visit, c_scale;
  double* sum;                      /* [n][m] in / out */
  int32_t* count;                   /* [n][m] in / out */
  int32_t* next_slot;               /* [n][k_next] out */
  int64_t* next_candidates;         /* [n][k_next] out */
} gvec_search_halve_args;
typedef struct gvec_search_policy_args {
  int32_t n, num_actions, m, reserved;
  const float* logits;              /* [n][num_actions], NULL = uniform over the legal set */
  const uint8_t* mask;              /* [n][num_actions] */
  const int64_t* candidates0;       /* [n][m] */
  const double* sum;                /* [n][m] */
  const int32_t* count;             /* [n][m] */
  const float* value;               /* [n], NULL = none */
  double q_lo, q_inv_range, c_visit, c_scale;
  float* target;                    /* [n][num_actions] out */
  float* v_mix;                     /* [n] out */
} gvec_search_policy_args;
int32_t gvec_search_halve(int32_t device, void* hip_stream, const gvec_search_halve_args* args);
int32_t gvec_search_improved_policy(int32_t device, void* hip_stream, const gvec_search_policy_args* args);

/* ---- tree search below the root: the full search of Danihelka et al. - sequential halving at the
 * root, the deterministic argmax(pi' - N / (1 + sum N)) rule at every node below it, one node expanded per simulation, values
 * backed up along the path.  The board of every node stays resident as an env of a scratch handle.
 *
 * gvec_search_expand: a playout launch that also KEEPS THE BOARD AFTER ITS FIRST TURN.  terms are exactly those of
 * gvec_search_playouts - of gvec_search_playouts_bot when bot_players or bot_random_permille is non-zero - on the same
 * arguments: the playout index, the key, the candidate decode, the invalid rows, the read-only roots and the depth turns.
 * On top, for every (root i, candidate k), replica 0's board as it stands after the playout's first turn is written into
 * env child_envs[i][k] of dst (child_envs device int32 [n][K]; NULL: env i*K + k).  Nothing is stored for a pair whose
 * entry is below 0 or at or above dst's num_envs (checked on the device, no host sync), for an invalid row, or when dst is
 * NULL - the call is then the plain playout launch.  status int32 [n][K], may be NULL: bit 0 a board was stored, bit 1 the
 * game is over after the first turn, bit 2 the seat is not alive after it; 0 for an invalid row.
 * Written to the destination env: the header except the slot's lifetime counters, which stay dst's own; the whole planes
 * block, types and lists included; the armies in the narrow or the wide form as every store picks it.  dst's legal-mask
 * buffer, error codes, recorded actions, gym baseline and experience rows are not touched.  The stored env equals env
 * (i*K + k)*R of gvec_search_playouts' own composition - the scratch handle of n*K*R copies, gvec_agent_actions(seed, 0)
 * (+ gvec_bot_actions), the candidate in the seat's slot, gvec_step - read after that first gvec_step: every field of
 * gvec_read_state, and every later call on dst behaves as if the env had always held that state.
 * dst must match h as gvec_copy_envs requires (plain handles, the same device, max dims and production constants):
 * GVEC_E_INVALID with the field named otherwise, and nothing is launched.  dst == h is allowed as long as no child env is
 * a root env of the same call (undefined otherwise, as for gvec_copy_envs).  Enqueued on h's stream, ordered after the work
 * already enqueued on dst's; dst's next call waits for it.  The other errors are gvec_search_playouts_bot's.
 *
 * The tree of row r < n has `nodes` nodes, node 0 the root, every node num_slots = C <= 64 child slots.  All arrays are
 * device memory and NODE-MAJOR ([nodes][n][C] and [nodes][n]), so that the root's slice is the [n][C] gvec_search_halve and
 * gvec_search_improved_policy take.  child_action GVEC_SEARCH_NONE marks an empty slot; child_node -1 = not expanded,
 * -2 = dead, else a node id; node_status bit 0 in use, bit 1 terminal.  A slot is OPEN when its action is not NONE and its
 * node is not dead.  Both entry points are handle-free: (device, hip_stream, args).
 *
 * gvec_tree_select: k columns per row, column c starting at root slot slot[r][c] (NULL: c, needs k == C; the slots of a
 * row are distinct).  A root slot outside [0, C) or a dead root edge gives leaf (0, -1).  A root edge that is not expanded
 * is the leaf (0, slot).  Otherwise the walk descends: at a terminal node, a node without an open slot or a node id
 * outside [0, nodes) it stops with leaf_slot = -1; at any other node u it picks a slot and stops there if that edge is not
 * expanded.  The pick, float64 over the open slots of u with N_c the slot's count, sumN their sum, nmax their maximum:
 *   pi = softmax(child_logit) (the maximum subtracted), q_c = sum_c / N_c where N_c > 0,
 *   v_mix = node_value[u] when sumN == 0, else (node_value[u] + sumN * (sum_{N>0} pi_c q_c / sum_{N>0} pi_c)) / (1 + sumN),
 *   qhat_c = q_c on visited slots, v_mix elsewhere,
 *   z_c = logit_c + ((c_visit + nmax) * c_scale) * ((qhat_c - q_lo) * q_inv_range)      (gvec_search_halve's grouping)
 *   pi' = softmax(z); the slot is argmax of pi'_c - N_c / (1 + sumN), the lowest slot on a tie.
 * Outputs [n][k]: leaf_node, leaf_slot, leaf_action (child_action of the leaf edge: the candidate to hand to
 * gvec_search_expand; GVEC_SEARCH_NONE when leaf_slot is -1) and leaf_depth (the leaf node's distance from the root).
 * The kernel reads the tree only.  One wavefront per (row, column), lane = slot; the sums are fixed butterflies.
 *
 * gvec_tree_backup: per column with leaf_slot >= 0, g = the mean PlayoutScore (gvec_search_halve's, operation for
 * operation) of the valid replicas of terms[r][c], added in order and divided once; with net_value, g = (1 - value_weight)
 * * g + value_weight * (double)net_value[r][c], in that order.  If bit 0 of status[r][c] is clear or no replica is valid
 * the leaf edge becomes dead (child_node -2) and nothing is added.  Otherwise the edge gets new_node[r][c] and that node
 * node_value = g, node_status = 1 | (status & 6 ? 2 : 0), its parent and slot.  A column that stopped at a terminal node
 * (leaf_slot -1, node_status bit 1, not the root) takes g = that node's node_value and starts at its parent edge.  From
 * that edge up to node 0, inclusive, child_sum += g and child_count += 1.  Every other column, and one whose leaf or
 * new_node is outside the tree, changes nothing.  Distinct root slots mean disjoint subtrees: no atomics, the same input
 * gives the same bits.  One wavefront per row, lane = column.
 * GVEC_E_INVALID with a message, before anything touches a device: args or a required pointer NULL (slot and net_value
 * may be), n < 0, num_slots outside [1, 64], k outside [1, num_slots] (select: slot NULL with k != num_slots), nodes < 1
 * or nodes * n at or above 2^31, replicas < 1, a non-zero reserved.  n == 0 is a no-op that needs no device. */
int32_t gvec_search_expand(gvec_handle* h, const gvec_search_args* args, uint32_t bot_players, int32_t bot_random_permille,
                           gvec_handle* dst, const int32_t* child_envs, int32_t* status);
typedef struct gvec_tree {
  int32_t n, nodes, num_slots, reserved;
  int64_t* child_action;            /* [nodes][n][C] */
  float* child_logit;               /* [nodes][n][C] */
  int32_t* child_node;              /* [nodes][n][C] */
  int32_t* child_count;             /* [nodes][n][C] */
  double* child_sum;                /* [nodes][n][C] */
  double* node_value;               /* [nodes][n] */
  int32_t* node_status;             /* [nodes][n] */
  int32_t* node_parent;             /* [nodes][n] */
  int32_t* node_slot;               /* [nodes][n] */
} gvec_tree;
typedef struct gvec_tree_select_args {
  gvec_tree tree;
  int32_t k, reserved;
  const int32_t* slot;              /* [n][k], NULL = identity */
  double q_lo, q_inv_range, c_visit, c_scale;
  int32_t* leaf_node;               /* [n][k] out */
  int32_t* leaf_slot;               /* [n][k] out */
  int64_t* leaf_action;             /* [n][k] out */
  int32_t* leaf_depth;              /* [n][k] out */
} gvec_tree_select_args;
typedef struct gvec_tree_backup_args {
  gvec_tree tree;
  int32_t k, replicas;
  const int32_t* leaf_node;         /* [n][k] */
  const int32_t* leaf_slot;         /* [n][k] */
  const int32_t* new_node;          /* [n][k] */
  const int32_t* terms;             /* [n][k][replicas][GVEC_SEARCH_TERMS] */
  const int32_t* status;            /* [n][k] */
  const float* net_value;           /* [n][k], NULL = none */
  double value_weight;
  double win, loss, land, army;     /* the score's weights */
} gvec_tree_backup_args;
int32_t gvec_tree_select(int32_t device, void* hip_stream, const gvec_tree_select_args* args);
int32_t gvec_tree_backup(int32_t device, void* hip_stream, const gvec_tree_backup_args* args);

/* ---- internal/experience side channel ------------------------------
 * gvec_experience_begin   = TurnProcessor.captureStateForExperience
 *                           (turn_processor.go:116-121: GameState.Clone before the step):
 *                           snapshots what the reward needs from the current state.
 * gvec_experience_rewards = CalculateReward(prev, cur, player) for every env / player
 *                           (internal/experience/rewards.go:40-85, DefaultRewardConfig
 *                           :23-37), prev = the snapshot, cur = the resident state;
 *                           rewards[B][max_players] float32, done[B] =
 *                           GameState.IsGameOver (state.go:73-82), may be NULL.  A board
 *                           that was re-dealt since the snapshot gets reward 0.
 * gvec_observe            = Serializer.StateToTensor(state, player)
 *                           (internal/experience/serializer.go:37-109): float32
 *                           [9][H][W] at index c*H*W + y*W + x inside a slot of
 *                           9*tile_stride floats; player >= 0: out[B][9*stride];
 *                           player = -1: out[B][max_players][9*stride].
 * gvec_serializer_mask    = Serializer.GenerateActionMask (serializer.go:112-176):
 *                           same packing as gvec_legal_mask but the serializer's
 *                           semantics (board owner, army >= 2, no Alive check) and
 *                           direction order 0 up, 1 down, 2 left, 3 right.
 * Alignment with GVEC_MEM_DEVICE: gvec_observe writes `out` in place and needs only the 4 bytes of a float (it picks
 * aligned 256-byte store windows, or per-slot stores, per env from the address and the env's own W*H).
 * gvec_serializer_mask writes `bits` in place as dwords: the array must be 4-BYTE aligned although it is declared as
 * bytes, and one that is not is refused with GVEC_E_INVALID and a gvec_last_error message before any launch. */
int32_t gvec_experience_begin(gvec_handle* h);
/* The same snapshot for envs [env_begin, env_begin+n) only (a consumer that samples a slice of the batch). */
int32_t gvec_experience_begin_range(gvec_handle* h, int32_t env_begin, int32_t n);
int32_t gvec_experience_rewards(gvec_handle* h, float* rewards, uint8_t* done, int32_t mem);

/* ---- configurable rewards: CalculateRewardWithConfig (internal/experience/rewards.go:45-85) with the caller's RewardConfig
 * (:8-20) instead of DefaultRewardConfig (:23-37).  The struct holds the NINE weights the Go function reads - TerritoryLost
 * and ArmyLost are never read there: a negative difference is multiplied by TerritoryGained / ArmyGained (:62, :68) - plus
 * what a gym env adds: invalid_action and the clip flag.
 *   win_game, lose_game              :49-56  a finished game with a winner: the value IS the reward (no shaped terms)
 *   territory                        :59-62  (tiles owned now - before) * TerritoryGained
 *   army                             :65-68  (armies owned now - before) * ArmyGained
 *   capture_city, lose_city          :71-73  countCityChanges :110-129
 *   capture_general, lose_general    :76-78  countGeneralChanges :132-151 (a captured general had an owner before)
 *   army_advantage                   :81-82  calculateArmyAdvantage :153-175 of the CURRENT state, in [-1, 1]
 *   flags bit 0 (GVEC_REWARD_CLIP)   NormalizeReward :215-223: the value clamped to [-1, 1]
 *   invalid_action                   added AFTER the clip where the learner's byte of `invalid` is set
 * float32, the reference's order of additions, no fused multiply-add: with gvec_reward_config_default the values equal
 * gvec_experience_rewards' bit for bit. */
#define GVEC_REWARD_CLIP 1u
typedef struct gvec_reward_config {
  float win_game, lose_game, capture_city, lose_city, capture_general, lose_general, territory, army, army_advantage;
  float invalid_action;
  uint32_t flags;     /* GVEC_REWARD_* */
  uint32_t reserved;  /* must be 0 */
} gvec_reward_config;
/* DefaultRewardConfig (rewards.go:23-37); invalid_action = 0, flags = 0. */
int32_t gvec_reward_config_default(gvec_reward_config* cfg);
/* A snapshot that holds only what the REWARD reads of the state before the step - every player's ownership plane and the
 * tail (territory, armies, turn, dimensions): about 250 bytes per env at 20x20 4P instead of gvec_experience_begin's 3.7 KB.
 * It is written into the same snapshot buffer and leaves the visibility, mask and army sections as they were: experience
 * RECORDS (gvec_experience_records) need the full gvec_experience_begin[_range]; after this call they would mix two turns.
 * gvec_experience_rewards and gvec_experience_rewards_config give the same values after either snapshot.  Sharded handles
 * fan out as gvec_experience_begin does. */
int32_t gvec_experience_begin_rewards(gvec_handle* h);
/* CalculateRewardWithConfig(prev, cur, p, cfg) for every env and every player of `players` (bit p = player p; 0 = all
 * max_players; a bit at or above max_players: GVEC_E_INVALID).  K = the number of players asked for; columns in ascending
 * player id.  Per (env, player):
 *   r = win_game / lose_game for a finished game with a winner, else the shaped sum in the order listed above;
 *   r = clamp(r, -1, 1) with GVEC_REWARD_CLIP;
 *   r = 0 for an env that was re-dealt or not stepped since the snapshot (gvec_experience_rewards' rule) and for p >= the
 *       env's own player count;
 *   r += invalid_action where invalid[env][k] != 0 (invalid: uint8 [B][K], may be NULL) - also on a row that was not stepped:
 *       a gym env that does not play a refused turn hands out exactly invalid_action.
 * Outputs, each may be NULL (all three NULL: GVEC_E_INVALID):
 *   rewards float32 [B][K]
 *   terms   int32   [B][K][8]: d_territory, d_army, cities gained, cities lost, generals gained, generals lost, outcome
 *           (+1 the winner of a finished game, -1 a loser, 0 otherwise), the army advantage's float32 bits; all zero where
 *           the reward is forced to 0.  What a caller recombines, or builds other shaping on.
 *   done    uint8   [B]: GameState.IsGameOver (state.go:73-82)
 * Refused with GVEC_E_INVALID and a gvec_last_error message before any launch: cfg NULL, a weight that is not finite,
 * reserved != 0, unknown flag bits, a players bit at or above max_players, all outputs NULL, no snapshot taken yet.
 * Sharded handles: host memory only, as gvec_experience_rewards. */
int32_t gvec_experience_rewards_config(gvec_handle* h, const gvec_reward_config* cfg, uint32_t players, const uint8_t* invalid,
                                       float* rewards, int32_t* terms, uint8_t* done, int32_t mem);

/* ---- experience records: what a rank ships to the process feeding StreamAggregator ----
 * One compact record per env transition = everything SimpleCollector.OnStateTransition
 * (internal/experience/collector.go:30-98) puts into the experiencepb.Experience of every player that
 * acted, with the two [9][H][W] float tensors per player replaced by what they are functions of:
 *   dword 0 currState.Turn | 1 W | H<<8 | P<<16 | flags<<24 (1 done = currState.IsGameOver, 2 fog of war,
 *   4 valid: the env was stepped, not re-dealt, since the snapshot) | 2 acted bits (bit p: player p
 *   submitted an action) | 3 env id (env_id_base + env) |
 *   action[MP] int32 (Serializer.ActionToIndex on prevState.Board.W, serializer.go:179-198; -1 none) |
 *   reward[MP] float32 (CalculateReward, rewards.go:40-85) |
 *   bit-planes of fd dwords (bit t = tile y*W+x): prev own[MP], prev visible[MP], next own[MP],
 *   next visible[MP], general, city, mountain |
 *   Serializer.GenerateActionMask(prevState, p) as [MP][4][fd] direction planes (0 up, 1 down, 2 left, 3 right) |
 *   prev armies, next armies: uint16[NS*64], tile t at halfword t, saturated to [0, 65535] - exact for
 *   StateToTensor, which clamps army/1000 at 1 (serializer.go:82-85).
 * MP / fd / NS come from gvec_experience_record_layout: out8 = {dwords per record, MP, fd, NS, max_players,
 * tile_stride, 0, 0}.  3,660 bytes at 20x20 4P instead of 115 KB of tensors; the consumer expands
 * (generalsreinforcementlearning_amd/experience.py: decode_records).
 * gvec_experience_records needs the snapshot of gvec_experience_begin[_range] taken BEFORE the step and the
 * actions[B][max_players] that were played (NULL = the handle's action buffer: the last host-mode
 * gvec_step, or the device agent's moves when gvec_record_agent_actions is on); it writes n records to
 * dst_device on the handle's stream. */
int32_t gvec_experience_record_layout(gvec_handle* h, int32_t* out8);
int32_t gvec_experience_record_bytes(gvec_handle* h);
int32_t gvec_experience_records(gvec_handle* h, const gvec_action* actions, int32_t mem, int32_t env_begin,
                                int32_t n, int32_t env_id_base, void* dst_device);
/* The CONSUMER side of the exchange (the GPU the records were gathered to, e.g. rank 0 feeding StreamAggregator or a
 * learner): expands n compact records (device memory on `device`) into the fields of the experiencepb.Experience messages
 * SimpleCollector.OnStateTransition builds (collector.go:41-75), one slot per (record, player), [n][MP] record-major,
 * MP = layout8[1] (layout8 as gvec_experience_record_layout fills it - the sender's; no engine handle is needed here):
 *   state, next_state  float32 [n][MP][9 * stride]: StateToTensor(prevState / currState, p), index c*H*W + y*W + x with
 *                      the record's own W, H at the start of the slot (stride = layout8[5]);
 *   action_mask        uint8   [n][MP][4 * stride]: GenerateActionMask(prevState, p) as 0/1 bytes, index t*4 + d,
 *                      d = 0 up, 1 down, 2 left, 3 right (the []bool of serializer.go:112-176);
 *   meta               int32   [n][MP][8]: present (1: the record is valid and player p acted - only then the slot
 *                      holds an experience, else it is zeroed), env id, player id, currState.Turn, action index, reward
 *                      (float32 bits), done, W | H << 8.
 * Enqueued on hip_stream (may be NULL) of `device`; device pointers only.  experience.py: expand_records_device.
 * Alignment: state / next_state / meta need what their types say (4 bytes; wider stores are chosen per slot from the
 * address).  `records` and `action_mask` must be 4-BYTE aligned although they are declared as bytes: a record is read as
 * dwords, and a tile's four mask bytes - as an absent slot's zeros - leave as one dword.  A pointer that is not is refused
 * with GVEC_E_INVALID and a gvec_last_error message before anything touches a device. */
int32_t gvec_expand_experience_records(int32_t device, void* hip_stream, const int32_t* layout8, const void* records, int32_t n,
                                       float* state, float* next_state, uint8_t* action_mask, int32_t* meta);
/* on != 0: per-turn rollouts (gvec_rollout fused = 0) store the agent's moves in the handle's action buffer and the
 * per-env error codes (the sentinel of the first failing move, 0, or GVEC_ERR_GAME_OVER) in its err buffer. */
int32_t gvec_record_agent_actions(gvec_handle* h, int32_t on);
int32_t gvec_observe(gvec_handle* h, int32_t player, float* out, int32_t mem);
int32_t gvec_serializer_mask(gvec_handle* h, uint8_t* bits, int32_t mem);

/* ---- the gRPC surface's per-turn broadcast --------------------------------------------------
 * gameInstance.createStreamUpdate (internal/grpc/gameserver/server.go:632-777) decides per env and player stream: when
 * 0 < |ChangedTiles| + |VisibilityChangedTiles| < W*H/5 the update is a GameStateDelta - the tiles of either set with the
 * proto's fog rules for that player (:664-689) plus every PlayerState - else the full GameState.  gvec_stream_deltas
 * makes that decision and builds the delta's tile updates on the device, so that a turn's broadcast reads back a few
 * eight-byte updates per env instead of the board:
 *   kind[B]    1 = delta, 2 = the server sends convertGameStateToProto's full state (gvec_read_state + gvec_player_visibility)
 *   count[B]   tile updates of the delta (0 for kind 2)
 *   updates    [B][cap] uint64, cap = gvec_stream_delta_cap(h) (= max(1, tile_stride / 5): a delta has fewer than N/5):
 *              bits 0-15 tile index y*W + x | 16-17 Tile.Type (core numbering, after the fog rules) | 18 visible |
 *              19 fog_of_war | 20-23 owner + 1 (0: -1, i.e. neutral or withheld) | 32-63 army (int32, 0 when withheld);
 *              the ChangedTiles in ascending order, then the tiles only in VisibilityChangedTiles (Go's map order is
 *              unspecified).  PlayerUpdates come from gvec_read_state's per-player fields (a few bytes per env).
 * GVEC_MEM_HOST or GVEC_MEM_DEVICE. */
int32_t gvec_stream_delta_cap(const gvec_handle* h);
int32_t gvec_stream_deltas(gvec_handle* h, int32_t player, uint8_t* kind, int32_t* count, uint64_t* updates, int32_t mem);
/* The same updates as ONE stream (host memory): env e's updates are updates[offset[e] .. offset[e + 1]), offset has B + 1
 * entries, *total = offset[B].  Only the updates that exist cross PCIe - about 11 per env-turn at 20x20 4P, 25 MB for
 * 262,144 boards instead of the 168 MB of the fixed-stride form or the 1 GB of the boards.  capacity = the entries
 * `updates` can hold: GVEC_E_RANGE (with *total set) when it is too small; B * gvec_stream_delta_cap(h) always suffices
 * (B * tile_stride with full_tiles).  full_tiles != 0: an env of kind 2 contributes ALL its W*H tiles in the same packed
 * form, ascending - the board of convertGameStateToProto's full state with the player's fog rules applied
 * (server.go:556-582) - so that a broadcast never reads a board back, growth turns included.  Plain handles only. */
int32_t gvec_stream_deltas_packed(gvec_handle* h, int32_t player, int32_t full_tiles, uint8_t* kind, int64_t* offset, uint64_t* updates,
                                  int64_t capacity, int64_t* total);

/* ---- python/generals_gym on the device ------------------------------------------
 * What GeneralsEnv builds on the client from the GameState proto of its player token, computed straight
 * from the resident state with the proto's fog rules (server.go:556-582) applied in the kernel.  Every
 * pointer is a DEVICE pointer (e.g. a torch tensor); work is enqueued on the handle's stream.
 * gvec_gym_observe: obs [B][9][tile_stride] float32 = GeneralsEnv._get_observation (generals_env.py:291-342:
 *   visible, ownership 0.5 / 1.0, log(army+1)/10, one-hot type, turn_count/max_turns, zeros), tile index
 *   y*W + x; mask [B][tile_stride*5] 0/1 bytes = _get_valid_actions_mask (:344-387), index tile*5 + {up, right,
 *   down, left, half}; reward [B] float64 = _calculate_reward (:499-561) against the player stats stored by
 *   the PREVIOUS gvec_gym_observe call of this handle (the call after a reset yields a meaningless reward);
 *   done = Engine.IsGameOver, winner = Engine.GetWinner.  reward / done / winner may be NULL.
 * gvec_gym_actions: GeneralsEnv.step's action handling (:226-259, :389-441) for `player`: decodes
 *   gym_actions[B] (indices into Discrete(board_size*5)) against `mask` (the last gvec_gym_observe's), writes
 *   the player's move into actions[B][max_players] (the other players' slots are kept: fill them first, e.g.
 *   with gvec_agent_actions), marks an env whose action is refused GVEC_ACT_SKIP_ENV and a `resetting` env
 *   GVEC_ACT_RESET_ENV; played / invalid / error [B] 0/1 outputs (any may be NULL).
 * Alignment (every gvec_gym_* call that writes obs / mask, the *_players ones included): obs needs the 4 bytes of a
 *   float, mask may sit at ANY byte address - slots of a larger buffer at element offsets are fine.  The kernels pick
 *   their store code per slot from the address and tile_stride (aligned 256-byte windows, 16-byte quads or one store per
 *   tile for obs; 16-byte, 4-byte or byte stores for mask); every choice writes the same bytes. */
int32_t gvec_gym_observe(gvec_handle* h, int32_t player, const int64_t* turn_count, int32_t max_turns,
                         float* obs, uint8_t* mask, double* reward, uint8_t* done, int8_t* winner);
/* gvec_gym_observe plus the bookkeeping GeneralsEnv.step wraps around it (generals_env.py:226-259), in the same
 * kernel: per env, with rs = resetting[env] (this step re-dealt it) and pl = played[env] (gvec_gym_actions accepted
 * the action): turn_count := rs ? 0 : turn_count + pl (in place, and copied to turn_out); the observation uses the new
 * count; reward := rs ? 0 : (pl ? _calculate_reward : -0.1); terminated := game over & pl & !rs; truncated :=
 * turn_count >= max_turns & pl & !rs; needs_reset := terminated | truncated; winner := terminated ? GetWinner : -1.
 * Outputs other than obs / mask may be NULL.  One launch instead of one launch and a dozen elementwise tensor ops. */
int32_t gvec_gym_finish_step(gvec_handle* h, int32_t player, int64_t* turn_count, int32_t max_turns,
                             const uint8_t* resetting, const uint8_t* played, float* obs, uint8_t* mask, double* reward,
                             uint8_t* terminated, uint8_t* truncated, int8_t* winner, uint8_t* needs_reset,
                             int64_t* turn_out);
int32_t gvec_gym_actions(gvec_handle* h, int32_t player, const int64_t* gym_actions, const uint8_t* mask,
                         const uint8_t* resetting, gvec_action* actions, uint8_t* played, uint8_t* invalid,
                         uint8_t* error);

/* GeneralsEnv.step (generals_env.py:226-259) for every env in ONE launch: exactly
 *   gvec_agent_actions(agent_seed, 0) -> gvec_gym_actions(gym_actions, the last observation's mask, resetting) ->
 *   gvec_step(device actions, no err / legal output) -> gvec_gym_finish_step(resetting, played, ...)
 * with the same outputs bit for bit, without the intermediate buffers: the learner's action is decoded against the
 * valid-action mask of the resident state (recomputed on the fly), the other players move like the on-device agent, the
 * turn is played and observation / mask / reward / flags of the new state are written while the board is in registers.
 * `resetting` = the needs_reset output of the previous call (zeros after a reset).  Needs auto_reset and a board pool
 * (GVEC_E_INVALID otherwise: a re-deal is how an episode ends here).  obs / mask / turn_count / gym_actions / resetting
 * are required, every other output may be NULL.  Device pointers only; enqueued on the handle's stream. */
int32_t gvec_gym_step(gvec_handle* h, int32_t player, uint64_t agent_seed, const int64_t* gym_actions, const uint8_t* resetting,
                      int64_t* turn_count, int32_t max_turns, float* obs, uint8_t* mask, double* reward, uint8_t* terminated,
                      uint8_t* truncated, int8_t* winner, uint8_t* needs_reset, int64_t* turn_out, uint8_t* played,
                      uint8_t* invalid, uint8_t* error);

/* Self-play: the gym calls for every learner of the bit set `learners` at once (bits below max_players; L = popcount,
 * per-learner arrays hold the learners in ascending player id: gym_actions / reward / invalid / error / alive [B][L],
 * obs [B][L][9][tile_stride], mask [B][L][tile_stride*5], every other array [B]).
 * gvec_gym_observe_players: gvec_gym_observe for each learner (the observation after a reset): obs, mask and reward per
 *   learner, done / winner per env, then every player's stats; plays no turn.  reward / done / winner may be NULL.
 * gvec_gym_step_players: gvec_gym_step for every learner in ONE launch.  Each learner's action is decoded against its own
 *   proto view as gvec_gym_step decodes the one learner's; the other players move like the on-device agent.  A refused
 *   action puts NO move in the learner's slot and the env still plays its turn (gvec_gym_step makes the env sit the call
 *   out instead): invalid / error [B][L] flag it and the learner's reward is _calculate_reward - 0.1.  A learner that is
 *   eliminated at the start of the step, or whose id is not below the env's player count, keeps invalid / error 0 and no
 *   penalty.  turn_count := resetting ? 0 : turn_count + 1; terminated / truncated / needs_reset / winner as gvec_gym_step
 *   with the turn played; reward 0 in a re-dealt (resetting) env; alive [B][L] = the learner's Player.Alive after the
 *   step.  With learners = 1 << p and every action accepted this equals gvec_gym_step(p) output for output.  Needs
 *   auto_reset and a board pool; plain handles only.  gym_actions / resetting / turn_count / obs / mask are required,
 *   every other output may be NULL.
 * Both share the stored player stats with gvec_gym_observe / gvec_gym_step: mixing single-learner and self-play calls on
 * one handle is consistent, because every one of them stores every player's stats. */
int32_t gvec_gym_observe_players(gvec_handle* h, uint32_t learners, const int64_t* turn_count, int32_t max_turns,
                                 float* obs, uint8_t* mask, double* reward, uint8_t* done, int8_t* winner);
int32_t gvec_gym_step_players(gvec_handle* h, uint32_t learners, uint64_t agent_seed, const int64_t* gym_actions,
                              const uint8_t* resetting, int64_t* turn_count, int32_t max_turns, float* obs, uint8_t* mask,
                              double* reward, uint8_t* terminated, uint8_t* truncated, int8_t* winner, uint8_t* needs_reset,
                              int64_t* turn_out, uint8_t* invalid, uint8_t* error, uint8_t* alive);

/* The collection loop around GeneralsEnv.step, resident on the device: one iteration of every worker's
 * ParallelEnvPool._run_episode (python/generals_gym/vector_env.py:164-192) plus ReplayBuffer.push
 * (python/generals_gym/replay_buffer.py:31-36) for num_envs workers, on the outputs of one gvec_gym_step, without a byte
 * crossing PCIe.  Per worker w, with live = !was_reset[w] (this step was not the worker's env.reset()):
 *   live:  the transition (state[w], action[w], reward[w], next_state[w], terminated[w] | truncated[w]) goes to the ring
 *          (workers in ascending order from the ring's cursor; the oldest transitions are overwritten once `capacity` is
 *          reached - deque(maxlen) semantics); episode_reward[w] += reward[w]; episode_length[w] += 1;
 *   over = live & (done | episode_length[w] >= max_steps_per_episode): (episode_reward, episode_length, w) is appended
 *          to the result log (vector_env.py:189-190; entries beyond result_capacity are counted, not kept), the two
 *          accumulators are zeroed, and needs_reset[w] is raised when the episode was cut at the length limit (so that
 *          the NEXT gvec_gym_step re-deals the env - the worker's next env.reset()).
 * ring_counters[4]  = {cursor, size, total pushed, 0};  pool_counters[4] = {episodes, results held, results dropped, 0}
 * (int64, device memory; zero them to start; "results held" is reset by the consumer after it has read the log).
 * scratch: gvec_pool_collect_scratch_bytes(num_envs) bytes, 16-byte aligned, contents of no interest to the caller.  Every
 * pointer is device memory on `device`; capacity >= num_envs.  Three launches on hip_stream: per-worker flags, one
 * workgroup's prefix counts (which also moves the counters on), the copy (a row of the ring is obs_floats floats, moved
 * by one to eight wavefronts). */
typedef struct gvec_collect_args {
  int32_t num_envs, obs_floats, max_steps_per_episode, reserved;
  int64_t capacity, result_capacity;
  const float* state; const float* next_state; const int64_t* action; const double* reward;
  const uint8_t* terminated; const uint8_t* truncated; const uint8_t* was_reset;
  uint8_t* needs_reset;
  float* ring_state; float* ring_next_state; int64_t* ring_action; double* ring_reward; uint8_t* ring_done;
  int64_t* ring_counters;
  double* episode_reward; int64_t* episode_length;
  double* result_reward; int32_t* result_length; int32_t* result_worker;
  int64_t* pool_counters;
  void* scratch;
} gvec_collect_args;
int32_t gvec_pool_collect(int32_t device, void* hip_stream, const gvec_collect_args* args);
uint64_t gvec_pool_collect_scratch_bytes(int32_t num_envs);

/* ---- prioritized experience replay over a ring in HBM (Schaul et al. 2016; the "Prioritized sampling support" of the
 * reference's documentation/MASTER_PLAN.md phase 3, which it never built) ----------------------------------------------
 * A radix-64 sum tree over the slots of a replay ring (the one gvec_pool_collect fills, or any other): float32, resident in
 * device memory, 256-byte aligned, gvec_per_tree_bytes(capacity) bytes.  Handle-free like gvec_pool_collect: every pointer
 * is DEVICE memory on `device`, work is enqueued on hip_stream, nothing synchronises.
 * Layout (gvec_per_tree_layout, in 4-byte words from the start of the tree): out[0] = L, the levels above the leaves;
 *   out[1] = the tree's size in words; out[2 + l] = first node of level l, l = 0 (one leaf per ring slot) .. L (the root).
 *   Node i of level l + 1 is the sum of nodes [64 i, 64 i + 64) of level l; levels are padded with zeros to a multiple of 64.
 *   The first GVEC_PER_HEADER_WORDS words are a header of uint32 words: GVEC_PER_HDR_MAX the running maximum of every leaf
 *   value ever written (a float's bits; starts at 1.0), _REJECTED how many updates were skipped (see below), _DRAWS the
 *   number of gvec_per_sample calls so far (the draw counter of its RNG; zero it to restart a seed's sequence - nothing
 *   else depends on it; the word after it is the kernels' own copy), _MIN0 two words and _SEQ two words of the kernels' own
 *   (the batch's smallest leaf, alternating by a call count a caller must leave alone).
 * A node is always recomputed from its 64 children, as the last term of the left-to-right float32 prefix the descent uses,
 *   so a slot whose leaf is 0 (no transition there) is never drawn and the tree cannot drift.
 * gvec_per_init: all leaves 0, maximum 1.0, counters 0.  One launch.
 * gvec_per_push: the rows appended to the ring between two copies of its counters {cursor, size, total pushed, 0} -
 *   `before` and `after`, device int64[4]; take `before` with a 32-byte device-to-device copy ahead of gvec_pool_collect and
 *   pass the live counters as `after` - get the running maximum as their leaf: slots [before.cursor, + after.pushed -
 *   before.pushed) mod capacity, all of them when the ring went round.  max_count sizes the launch (the host does not
 *   know the count): rows beyond it keep their leaves and _REJECTED goes up by one.  Two launches.
 * gvec_per_update: leaf[idx[i]] = (|td[i]| + eps) ** alpha for i < n (float32), the maximum moves, every ancestor is
 *   refreshed.  Duplicate indices: one of the supplied values wins.  An index outside [0, capacity), or an error that is
 *   NaN or infinite, is skipped and counted in _REJECTED (checked on the device).  A slot the ring has overwritten since it
 *   was drawn simply takes the stale priority, as in standard prioritized replay.  1 + (levels of more than 64 nodes) + 1
 *   launches: 4 for 16 M slots.
 * gvec_per_sample: k stratified draws with replacement: draw j aims at (j + u[j]) / k * total, formed in float64, and
 *   descends in float32.  u: k float64 in [0, 1), or NULL for the build's counter RNG keyed by (seed, _DRAWS, j), 53 bits a
 *   draw.  idx[k] int64, weight[k] float32 = (size * leaf / total) ** -beta over the batch's largest such value (= (leaf /
 *   the batch's smallest leaf) ** -beta: size and total cancel); ring_counters (the ring's live counters) says whether the
 *   ring holds anything: an empty ring or tree gives idx -1 and weight 0.  Two launches.
 * GVEC_E_INVALID (with a gvec_last_error message) before anything touches a device: tree NULL or not 256-byte aligned,
 *   capacity < 1 or > 2^36, n < 0, k < 1, max_count < 1, alpha < 0, beta < 0, eps <= 0 (NaN included), another required
 *   pointer NULL.  n == 0 is a no-op that needs no device. */
#define GVEC_PER_HEADER_WORDS 64
#define GVEC_PER_HDR_MAX      0
#define GVEC_PER_HDR_REJECTED 1
#define GVEC_PER_HDR_DRAWS    2
#define GVEC_PER_HDR_MIN0     4
#define GVEC_PER_HDR_SEQ      6
uint64_t gvec_per_tree_bytes(int64_t capacity);
int32_t gvec_per_tree_layout(int64_t capacity, int64_t* out10);
int32_t gvec_per_init(int32_t device, void* hip_stream, void* tree, int64_t capacity);
int32_t gvec_per_push(int32_t device, void* hip_stream, void* tree, int64_t capacity, const int64_t* counters_before,
                      const int64_t* counters_after, int64_t max_count);
int32_t gvec_per_update(int32_t device, void* hip_stream, void* tree, int64_t capacity, const int64_t* idx, const float* td_error,
                        int64_t n, float alpha, float eps);
int32_t gvec_per_sample(int32_t device, void* hip_stream, void* tree, int64_t capacity, const int64_t* ring_counters, int64_t k,
                        float beta, const double* u, uint64_t seed, int64_t* idx, float* weight);

/* ---- n-step returns over the replay ring ("Multi-step Learning", n_step = 3, of the reference's
 * documentation/claude/training-next-steps.md section 3.1, which it never built) -----------------------
 * gvec_pool_collect appends only the live workers' rows, compacted from the cursor, so the distance in the ring between a
 * worker's step t and its step t + 1 changes every step, and a cut at max_steps_per_episode leaves done = 0 in the ring.  Two
 * arrays record what the ring does not.  ring_succ: int64 [capacity]; ring_succ[s] is the slot that holds the same worker's
 * next transition of the same episode, or -1: that transition does not exist yet, the episode ended with row s (terminated |
 * truncated, or cut at the limit - the collector's `over`), or the row was not written by the collector.  nstep_last: int64
 * [num_envs][2], {global sequence number, slot} of each worker's latest row while its episode is open, {-1, -1} otherwise;
 * a row's global sequence number is the ring's "total pushed" counter at the moment it was appended.  Fill both with -1 to
 * start; a caller that writes rows by itself sets ring_succ = -1 for them.  Handle-free like gvec_pool_collect: every pointer
 * is DEVICE memory on `device`, work is enqueued on hip_stream, nothing synchronises, the host never learns the row count.
 * gvec_nstep_link: call it right after gvec_pool_collect, on the same stream, with the SAME args.  Ordering contract: it
 *   reads only num_envs, capacity, ring_counters and scratch of args, and what that call left in args->scratch (every worker's live / over flags and the per-group prefix counts of the live
 *   ones), so it must run after that gvec_pool_collect and before the next call that uses the same scratch, and nothing else
 *   may append to the ring between the two.  counters_before: a copy of ring_counters taken ahead of gvec_pool_collect - the
 *   32-byte device-to-device copy gvec_per_push wants, so one copy serves both; args->ring_counters holds the counters after.
 *   For every live worker w (its step was not its reset: the live flag of the scratch), whose new row has sequence q = before.pushed + (live workers below w)
 *   and slot s = (before.cursor + that count) mod capacity: if nstep_last[w] is open and its row is still held -
 *   prev_seq >= after.pushed - capacity, decided by this arithmetic alone, never by reading the slot, which this very step's
 *   push may have rewritten - then ring_succ[prev_slot] = s; ring_succ[s] = -1; nstep_last[w] = over ? {-1, -1} : {q, s}.
 *   A worker whose step was its reset writes nothing.  A predecessor that is still held is never one of this step's slots,
 *   so no two workers write one word.  One launch, one thread per worker.
 * gvec_nstep_gather: the whole batch for k sampled slots idx[k] (from any draw; gvec_per_sample's included) in one launch.
 *   Per sample, every float64 operation in exactly this order (no fused multiply-add: a float64 loop on the host
 *   reproduces ret and discount bit for bit):
 *     cur = idx; ret = reward[cur]; disc = 1.0; steps = 1
 *     while steps < n_step and !done[cur] and succ[cur] >= 0:
 *       cur = succ[cur]; disc = disc * gamma; ret = ret + disc * reward[cur]; steps += 1
 *     discount = disc * gamma
 *   Outputs: state[k] = ring_state[idx], next_state[k] = ring_next_state[cur], action[k] = ring_action[idx], ret[k],
 *   discount[k] (= gamma ** steps by the repeated product), done[k] = ring_done[cur], steps[k], last_idx[k] = cur.  A
 *   learner's target is ret + discount * (1 - done) * max Q(next_state).  An index outside [0, size) - the -1 of an empty
 *   prioritized tree included - gives steps 0, ret 0, discount 0, done 0, action -1, last_idx -1 and zero-filled rows.  A link
 *   that points outside [0, capacity) ends the walk like -1.  ring_succ may be NULL only when n_step == 1 (then ret = reward,
 *   discount = gamma).  1 << s wavefronts per sample, s the smallest of 0..3 with k << s >= 16384 (else 3) - the rule of
 *   gvec_pool_collect's copy, from the row count alone; the walk costs at most n_step - 1 dependent loads per wavefront,
 *   the two rows - which come from two different slots - move with 16-byte loads and stores aligned on both sides.
 * GVEC_E_INVALID (with a gvec_last_error message) before anything touches a device: args or a required pointer NULL,
 *   capacity < 1, k < 0 or > 2^28, n_step < 1, obs_floats < 1, gamma not finite or negative, ring_succ NULL with n_step > 1; for the
 *   link call also num_envs < 1 or num_envs > capacity, and a scratch that is not 16-byte aligned.  k == 0 is a no-op that
 *   needs no device. */
typedef struct gvec_nstep_gather_args {
  int64_t k, capacity;
  int32_t n_step, obs_floats;
  double gamma;
  const int64_t* idx;
  const float* ring_state; const float* ring_next_state; const int64_t* ring_action; const double* ring_reward;
  const uint8_t* ring_done; const int64_t* ring_counters; const int64_t* ring_succ;
  float* state; float* next_state; int64_t* action; double* ret; double* discount; uint8_t* done; int32_t* steps;
  int64_t* last_idx;
} gvec_nstep_gather_args;
int32_t gvec_nstep_link(int32_t device, void* hip_stream, const gvec_collect_args* args, const int64_t* counters_before,
                        int64_t* ring_succ, int64_t* nstep_last);
int32_t gvec_nstep_gather(int32_t device, void* hip_stream, const gvec_nstep_gather_args* args);

/* ---- on-policy self-play rollouts: trajectory store, GAE, minibatch gather (PPO) ---------------------
 * A rollout of T steps over N = num_envs * num_learners streams, learner-minor - exactly the [B][L] order
 * gvec_gym_step_players emits.  Handle-free like gvec_pool_collect: every pointer is DEVICE memory on `device`, work is
 * enqueued on hip_stream, nothing synchronises.  Precondition: every board holds max_players players (the boards
 * GeneralsSelfPlayVecEnv deals), so that `alive` of a learner means what it says in every env.
 * Row t describes step t: reset[b] is that step's `resetting` INPUT (the env was re-dealt and the action ignored),
 * terminated[b] / truncated[b] its outputs, alive[b][l] the learner's Player.Alive after it.  alive_state u8[N] persists
 * between steps and rollouts: `alive` after the previous step, all ones after a reset of the envs.
 * gvec_traj_record, one launch per step: row t of action int64[T][N], logp float32[T][N], value float32[T+1][N], reward
 *   float64[T][N] and flags uint8[T][N] from the step's [N] / [B] arrays, then alive_state := alive.
 *     GVEC_TRAJ_VALID    = !reset & alive_state                   the row is a transition of a learner still in the game
 *     GVEC_TRAJ_TERMINAL = VALID & (terminated | !alive)          no bootstrap past this row (elimination ends that learner)
 *     GVEC_TRAJ_CUT      = VALID & (terminated | truncated | !alive)   the advantage recursion stops here
 * gvec_traj_gae: generalized advantage estimation, backwards over t = T-1 .. 0 per stream, in float64; next_v = value[t+1]
 *   and value[T] is the caller's bootstrap:
 *     valid row    delta = reward + gamma * (TERMINAL ? 0 : next_v) - value[t]
 *                  adv[t] = delta + gamma * lambda * (CUT ? 0 : adv[t+1]);   ret[t] = adv[t] + value[t]
 *     invalid row  adv = 0, ret = value[t], and the carried advantage is cleared
 *   A truncated episode needs no special case: row t+1 of a truncated env is its re-deal row, and value[t+1] was evaluated
 *   on the final observation the truncating step returned - the bootstrap wanted.  adv / ret float32[T][N], rounded once.
 *   stats double[4] = {valid rows, sum of adv, sum of adv^2, 0} over the valid rows, of adv AS STORED (float32), by a
 *   fixed-order two-stage reduction without atomics: the same input gives the same bits.  Two launches.
 * gvec_traj_vtrace: V-trace targets (Espeholt et al., IMPALA, 2018) for a rollout whose acting policy mu is not the policy
 *   pi that is trained: the same backward recurrence over the same flags, with one more input per row, the learner's
 *   log-prob of the stored action.  Per stream, backwards over t = T-1 .. 0, in float64; V[t] = (double)value[t] and
 *   value[T] is the caller's bootstrap:
 *     w   = exp((double)logp_target[t] - (double)logp_behaviour[t])           the two float32 log-probs
 *     rho = min(rho_bar, w);   c = min(c_bar, w);   gl = gamma * lambda, formed once
 *     valid row    nv    = TERMINAL ? 0 : V[t+1]
 *                  nvs   = TERMINAL ? 0 : (CUT ? V[t+1] : vs_next)       vs_next: the UNROUNDED vs of row t+1; V[T] for t = T-1
 *                  delta = rho * ((reward + gamma * nv) - V[t])
 *                  acc   = delta + (gl * c) * (CUT ? 0 : acc_next)
 *                  vs[t] = V[t] + acc
 *                  pg[t] = rho * ((reward + gamma * nvs) - V[t])
 *                  rho_out[t] = rho
 *     invalid row  acc = 0, vs[t] = V[t], pg[t] = 0, rho_out[t] = 0
 *     then acc_next = acc, vs_next = vs[t]
 *   A CUT row bootstraps pg from V[t+1], as delta does: vs of row t+1 carries the corrections of the rows after the cut,
 *   which are no part of this episode (after a truncation row t+1 is the re-deal row and the two agree; flags from
 *   elsewhere may put a valid row there).  With logp_target bitwise
 *   equal to logp_behaviour and both bars >= 1, vs is gvec_traj_gae's ret exactly (before the rounding), and with lambda = 1
 *   as well pg is its adv up to rounding.  vs / pg / rho_out float32[T][N], each rounded once; rho_out may be NULL.
 *   stats double[4] = {valid rows, sum of pg, sum of pg^2, sum of rho_out} over the valid rows of the values AS STORED, by
 *   the same fixed-order two-stage reduction: slots 0-2 mean what gvec_traj_gather reads, which normalises pg unchanged.
 *   rho_bar / c_bar = +inf: no clipping.  Two launches.
 * gvec_traj_compact: idx int64[T*N] takes the ascending positions p = t*N + n of the VALID rows, *count their number
 *   (entries of idx beyond it are left alone).  Three launches.
 * gvec_traj_gather: the minibatch of M positions pos[i] in [0, T*N): out_obs[i] = the obs_floats floats of row pos[i] of
 *   the [T+1][N][obs_floats] observation store, out_mask[i] its mask_bytes bytes of the mask store (mask_bytes == 0: no
 *   masks, the two pointers unused), action / logp / value / ret copied, out_adv = adv, or with stats != NULL
 *   (adv - mean) / sqrt(var + 1e-8) in float64 with mean = stats[1] / stats[0], var = max(stats[2] / stats[0] - mean^2, 0)
 *   (both 0 when stats[0] == 0); out_weight float32 = VALID ? 1 : 0.  A position outside the range gives a zeroed row with
 *   weight 0 and adds one to *rejected (checked on the device).  Rows need only 4-byte (masks: 1-byte) alignment.  One launch,
 *   one to eight wavefronts per row.
 * scratch (gae, vtrace, compact): gvec_traj_scratch_bytes(T, N) bytes, 16-byte aligned, contents of no interest to the caller.
 * GVEC_E_INVALID (with a gvec_last_error message) before anything touches a device: args or a required pointer NULL,
 *   T < 1, N < 1 (num_envs < 1, num_learners < 1), t outside [0, T), M < 0, gamma or lambda outside [0, 1] (NaN included),
 *   rho_bar or c_bar not > 0 (NaN included), obs_floats < 1, mask_bytes < 0.  M == 0 is a no-op that needs no device. */
#define GVEC_TRAJ_VALID    1
#define GVEC_TRAJ_TERMINAL 2
#define GVEC_TRAJ_CUT      4
typedef struct gvec_traj_record_args {
  int64_t T, t;
  int32_t num_envs, num_learners;
  const int64_t* step_action; const float* step_logp; const float* step_value; const double* step_reward;   /* [N] */
  const uint8_t* reset; const uint8_t* terminated; const uint8_t* truncated;                                /* [B] */
  const uint8_t* alive;                                                                                     /* [N] */
  uint8_t* alive_state;                                                                                     /* [N] in / out */
  int64_t* action; float* logp; float* value; double* reward; uint8_t* flags;                               /* the stores */
} gvec_traj_record_args;
typedef struct gvec_traj_gae_args {
  int64_t T, N;
  double gamma, lambda;
  const double* reward; const float* value; const uint8_t* flags;
  float* adv; float* ret;
  double* stats;
  void* scratch;
} gvec_traj_gae_args;
typedef struct gvec_traj_vtrace_args {
  int64_t T, N;
  double gamma, lambda, rho_bar, c_bar;
  const double* reward; const float* value; const uint8_t* flags;
  const float* logp_behaviour; const float* logp_target;                                   /* [T][N] */
  float* vs; float* pg;
  float* rho_out;                                                                          /* NULL: not stored */
  double* stats;
  void* scratch;
} gvec_traj_vtrace_args;
typedef struct gvec_traj_compact_args {
  int64_t T, N;
  const uint8_t* flags;
  int64_t* idx; int64_t* count;
  void* scratch;
} gvec_traj_compact_args;
typedef struct gvec_traj_gather_args {
  int64_t T, N, M;
  int32_t obs_floats, mask_bytes;
  const int64_t* pos;
  const float* obs; const uint8_t* mask;
  const int64_t* action; const float* logp; const float* value; const float* ret; const float* adv; const uint8_t* flags;
  const double* stats;                                                                     /* NULL: adv as stored */
  float* out_obs; uint8_t* out_mask;
  int64_t* out_action; float* out_logp; float* out_value; float* out_ret; float* out_adv; float* out_weight;
  int64_t* rejected;
} gvec_traj_gather_args;
uint64_t gvec_traj_scratch_bytes(int64_t T, int64_t N);
int32_t gvec_traj_record(int32_t device, void* hip_stream, const gvec_traj_record_args* args);
int32_t gvec_traj_gae(int32_t device, void* hip_stream, const gvec_traj_gae_args* args);
int32_t gvec_traj_vtrace(int32_t device, void* hip_stream, const gvec_traj_vtrace_args* args);
int32_t gvec_traj_compact(int32_t device, void* hip_stream, const gvec_traj_compact_args* args);
int32_t gvec_traj_gather(int32_t device, void* hip_stream, const gvec_traj_gather_args* args);

/* ---- masked-categorical policy head: sample, evaluate, backward (PPO) -----------------------------
 * What stands between a network's logits and gvec_traj_record.  Handle-free like gvec_traj_*: every pointer is DEVICE memory
 * on `device`, work is enqueued on hip_stream, nothing synchronises.  A row is num_actions = A float32 logits and A mask
 * bytes (nonzero = legal; a bool tensor as it is); rows are dense ([rows][A]) and need only their dtype's alignment.
 * Logits are finite or -inf; NaN and +inf are the caller's error and may propagate.  Per row, with S = {i : mask_i != 0 and
 * l_i > -inf}:  m = max_S l_i,  Z = sum_S exp(l_i - m),  logp_i = l_i - m - log Z,  p_i = exp(logp_i),  H = -sum_S p_i logp_i.
 * A row with S empty is DEAD (no legal action, or every legal logit -inf): action 0, logp 0, entropy 0, zero gradients, never
 * a NaN.  |S| = 1 gives logp = 0 and H = 0 exactly.  float32 throughout, fixed reduction orders: the same input gives the same
 * bits on every call.  One wavefront per row; a row of A <= 5120 is read from HBM once.
 * gvec_policy_sample: action int64[rows], logp float32[rows] (of that action), entropy float32[rows].  greedy == 0: Gumbel-max,
 *   action = argmax_S (l_i + g_i), lowest index among equals, g_i = -log(-log u_i) from the build's counter RNG keyed by
 *   (seed, row_base + r, i) - DESIGN.md section 6 "Policy head" has the formula.  A draw depends on nothing else: rows
 *   [R/2, R) sampled alone with row_base = R/2 repeat the second half of the full call.  greedy != 0: argmax_S l_i, lowest
 *   index among equals.
 * gvec_policy_evaluate: logp[r] = logp_{action[r]} and entropy[r].  An action outside [0, A) or outside S has logp 0 and adds
 *   one to *bad_actions (int64, may be NULL; a device atomic, as gvec_traj_gather's `rejected`) - except on a dead row, where
 *   no action is legal and none is counted.
 * gvec_policy_backward: grad_logits float32[rows][A], EVERY element written (no clearing needed), p recomputed from the
 *   logits:  i in S: grad_logp[r] * (1[i == action[r]] - p_i) - grad_entropy[r] * p_i * (logp_i + H);  otherwise 0.
 *   grad_logp / grad_entropy float32[rows], either may be NULL (= zeros).  An action outside S carries no logp gradient.
 * GVEC_E_INVALID (with a gvec_last_error message) before anything touches a device: args or a required pointer NULL,
 *   num_actions < 1, rows < 0 or rows >= 2^31.  rows == 0 is a no-op that needs no device. */
typedef struct gvec_policy_sample_args {
  int64_t rows;
  int32_t num_actions, greedy;
  uint64_t seed;
  int64_t row_base;
  const float* logits; const uint8_t* mask;
  int64_t* action; float* logp; float* entropy;
} gvec_policy_sample_args;
typedef struct gvec_policy_evaluate_args {
  int64_t rows;
  int32_t num_actions, reserved;
  const float* logits; const uint8_t* mask; const int64_t* action;
  float* logp; float* entropy;
  int64_t* bad_actions;                                                                    /* NULL: not counted */
} gvec_policy_evaluate_args;
typedef struct gvec_policy_backward_args {
  int64_t rows;
  int32_t num_actions, reserved;
  const float* logits; const uint8_t* mask; const int64_t* action;
  const float* grad_logp; const float* grad_entropy;                                       /* NULL: zeros */
  float* grad_logits;
} gvec_policy_backward_args;
int32_t gvec_policy_sample(int32_t device, void* hip_stream, const gvec_policy_sample_args* args);
int32_t gvec_policy_evaluate(int32_t device, void* hip_stream, const gvec_policy_evaluate_args* args);
int32_t gvec_policy_backward(int32_t device, void* hip_stream, const gvec_policy_backward_args* args);

/* ---- policy distillation: masked soft-target cross-entropy / KL against a search's policy target ----
 * The loss that trains the prior on what gvec_search_improved_policy wrote.  Same conventions, same rows, same S, m, Z, logp_i,
 * p_i, H and the same reduction orders as the policy head above (the kernels share its code, operation for operation).
 * target float32[rows][A] needs no normalisation.  Per row:
 *   tau_i = target_i where i in S and target_i > 0, otherwise 0: mass on illegal actions, negative and NaN entries are dropped
 *           (nothing is counted, nothing synchronises);
 *   Tsum = sum_i tau_i;
 *   ce = -sum_{tau_i > 0} tau_i * logp_i;
 *   kl = sum_{tau_i > 0} tau_i * (log tau_i - logp_i), a sum of its own (not ce - H(tau)): >= 0 up to rounding when Tsum = 1;
 *   entropy = H.
 * A dead row gives ce = kl = entropy = 0.  A one-hot target at a legal action a gives ce = -logp_a with the bits of
 * gvec_policy_evaluate; |S| = 1 gives ce = 0; an all-zero target gives ce = kl = 0.
 * gvec_policy_distill: ce, kl, entropy float32[rows], every element written.
 * gvec_policy_distill_backward: grad_logits float32[rows][A], EVERY element written, everything recomputed from the inputs.
 *   With g = grad_ce[r] + grad_kl[r] (d kl / d logits = d ce / d logits: the target is a constant and gets no gradient):
 *   i in S: g * (Tsum * p_i - tau_i) - (grad_entropy[r] * p_i) * (logp_i + H);  otherwise, and on a dead row, 0.
 *   grad_ce / grad_kl / grad_entropy float32[rows], each may be NULL (= zeros).  |S| = 1 gives exact zeros.
 * A row of A <= 5120 reads logits, mask and target from HBM once per kernel (9 A bytes forward, 13 A backward with the
 * gradient's store); a longer row reads them again in every pass.
 * GVEC_E_INVALID (with a gvec_last_error message) before anything touches a device: args NULL, num_actions < 1, rows < 0 or
 *   rows >= 2^31, or rows > 0 and a required pointer NULL.  rows == 0 is a no-op that needs no device. */
typedef struct gvec_policy_distill_args {
  int64_t rows;
  int32_t num_actions, reserved;
  const float* logits; const uint8_t* mask; const float* target;
  float* ce; float* kl; float* entropy;
} gvec_policy_distill_args;
typedef struct gvec_policy_distill_backward_args {
  int64_t rows;
  int32_t num_actions, reserved;
  const float* logits; const uint8_t* mask; const float* target;
  const float* grad_ce; const float* grad_kl; const float* grad_entropy;                   /* NULL: zeros */
  float* grad_logits;
} gvec_policy_distill_backward_args;
int32_t gvec_policy_distill(int32_t device, void* hip_stream, const gvec_policy_distill_args* args);
int32_t gvec_policy_distill_backward(int32_t device, void* hip_stream, const gvec_policy_distill_backward_args* args);

/* ---- strategic feature planes: a pure function of the observation ------------------------------------
 * Five planes a small conv torso cannot compute for itself, from the nine planes of any observation: what a step returned, a
 * replay or rollout minibatch.  Handle-free like the policy head: DEVICE pointers on `device`, enqueued on hip_stream, nothing
 * synchronises.  Nothing is read that the observation does not hold, so no fog leaks.
 * obs float32 [rows][9][H*W], consecutive observations obs_row_stride floats apart; tile t = y*W + x.  Per tile:
 *   vis = obs[0] != 0, mine = obs[1] == 0.5, enemy = obs[1] == 1.0, mtn = obs[4] != 0, city = obs[5] != 0, gen = obs[6] != 0,
 *   pass = !mtn.  Planes 2, 3, 7 and 8 are not read.
 * out float32 [rows][5][H*W], contiguous, EVERY element written.  Planes 0-3 hold min(d, cap) / cap, d the length of the
 *   shortest 4-connected path from the tile to a source tile of the plane over passable tiles (both ends included; no step
 *   wraps from column W-1 to column 0 of the next row).  A source has d = 0; an impassable or unreachable tile, and every tile
 *   of a plane without a source, gets 1.0.  Sources: 0 gen & mine (the own general), 1 enemy, 2 city & !mine (cities to take),
 *   3 !vis & pass (the nearest fogged tile).  Plane 4, the front line: 1.0 where mine holds and a 4-neighbour is enemy, else 0.0.
 *   cap is a power of two, so every value is an exact float32: the result is defined to the bit.
 * GVEC_E_INVALID (with a gvec_last_error message) before anything touches a device: args or a required pointer NULL,
 *   rows < 0 or rows >= 2^31, width or height outside [1, GVEC_MAX_DIM], cap not a power of two in [2, 1024], reserved != 0,
 *   obs_row_stride < 9*width*height.  rows == 0 is a no-op that needs no device. */
typedef struct gvec_obs_features_args {
  int64_t rows;
  int32_t width, height, cap, reserved;
  int64_t obs_row_stride;                                                                  /* floats, >= 9*width*height */
  const float* obs; float* out;
} gvec_obs_features_args;
int32_t gvec_obs_features(int32_t device, void* hip_stream, const gvec_obs_features_args* args);

/* ---- fog-of-war memory planes: what a learner last saw of every tile -----------------------------------
 * An observation shows owner and army of the tiles visible this turn only.  A memory row keeps, per tile, what the learner's
 * last sight of it showed and how long ago that was: state that outlives one observation, carried by the caller from update to
 * update.  Handle-free like the feature planes: DEVICE pointers on `device`, enqueued on hip_stream, nothing synchronises.
 * One memory row, float32 [4][H*W], belongs to one learner's view; tile t = y*W + x:
 *   0 seen        1.0 once the tile has been visible in this episode, else 0.0
 *   1 last_owner  plane 1 of the observation in which the tile was last visible (0.5 mine, 1.0 somebody else's, 0.0 nobody's)
 *   2 last_army   plane 2 (log(army + 1) / 10) of that same observation
 *   3 age         min(k, cap) / cap, k the number of updates since the tile was last visible: 0 while it is visible, 1.0 while
 *                 seen is 0
 * The blank row is seen = 0, last_owner = 0, last_army = 0, age = 1.0.
 * One update, (prev, obs, reset) -> out, per row r and tile:
 *   base = the blank row when prev is NULL or reset[r / rows_per_flag] != 0, else prev[r].
 *   visible (obs[r][0] != 0):  seen = 1.0, last_owner = obs[r][1], last_army = obs[r][2] (both copied bit for bit), age = 0.0.
 *   not visible:               seen, last_owner and last_army are base's; age = min(base.age * cap + 1, cap) / cap when
 *                              base.seen != 0, else 1.0.
 * Planes 3 to 8 of the observation are not read.  EVERY element of out is written.  cap is a power of two, so every age is an
 * exact float32 and base.age * cap an exact integer: the result is defined to the bit.
 * obs float32 [rows][9][H*W], consecutive observations obs_row_stride floats apart; prev and out float32 [rows][4][H*W], dense.
 * prev == out (in place) is allowed: a tile's result depends on that tile's inputs alone.  reset uint8 [rows / rows_per_flag]:
 * one flag per rows_per_flag consecutive rows (the learners of one self-play env share its re-deal flag); NULL = no row restarts.
 * GVEC_E_INVALID (with a gvec_last_error message) before anything touches a device: args, obs or out NULL, rows < 0 or
 *   rows >= 2^31, width or height outside [1, GVEC_MAX_DIM], cap not a power of two in [2, 1024], rows_per_flag < 1 or not a
 *   divisor of rows, obs_row_stride < 9*width*height, prev overlapping out without being equal to it.  rows == 0 is a no-op
 *   that needs no device. */
typedef struct gvec_obs_memory_args {
  int64_t rows;
  int32_t width, height, cap, rows_per_flag;
  int64_t obs_row_stride;                                                                  /* floats, >= 9*width*height */
  const float* obs;
  const float* prev;                                                                       /* NULL: every row starts blank */
  const uint8_t* reset;                                                                    /* NULL: no row restarts */
  float* out;
} gvec_obs_memory_args;
int32_t gvec_obs_memory_update(int32_t device, void* hip_stream, const gvec_obs_memory_args* args);

/* ---- masked Q targets from next observations: Double DQN and categorical (C51) ----------------------
 * A replay row holds (s, a, r, ns, d) and no legal-action mask of ns; the mask is a pure function of ns, so the bootstrap can
 * run over the legal actions alone.  Handle-free like the feature planes: DEVICE pointers on `device`, enqueued on hip_stream,
 * nothing synchronises.  Observations are float32 [rows][9][H*W], obs_row_stride floats apart, tile t = y*W + x; A = 5*H*W.
 * The legal set S of an observation (GeneralsEnv._get_valid_actions_mask restated on planes 1, 2 and 4, the others unread):
 *   tile t is a source iff obs[1][t] == 0.5 and obs[2][t] > 0.09 (an army of 1 shows as ln(2)/10 = 0.0693, of 2 as 0.1099);
 *   a tile is passable iff obs[4][tile] == 0;  action 5*t + d, d < 4 (up, right, down, left: (x, y-1), (x+1, y), (x, y+1),
 *   (x-1, y)), is legal iff t is a source and that neighbour is on the board and passable;  5*t + 4 (the half move) iff any of
 *   the four is.
 * The argmax of both targets: over i in S in any order, i wins iff v_i > best or (v_i == best and i < index), starting from
 *   (-inf, none): the greatest value, the lowest index among equals; a NaN never wins; an all -inf legal set picks its lowest.
 * Values at actions outside S are never loaded: they may hold anything.  discount float32 [rows] (gamma ** steps of an n-step
 * row), or NULL = the scalar gamma for every row.  done uint8 [rows].  The same input gives the same bits on every call.
 * gvec_obs_valid_mask: mask uint8 [rows][A], 1 where the action is in S else 0 - the bytes of info["valid_actions_mask"].
 * gvec_q_target: q_eval, q_select float32 [rows][A]; q_select NULL = q_eval (plain masked DQN; given = Double DQN).
 *   a* = argmax_S q_select.  next_action int64 [rows] = a*, or -1 when nothing won.  When nothing won or done[r] != 0:
 *   next_value = 0 and target = reward[r].  Otherwise next_value = q_eval[a*], target = reward + discount * next_value: one
 *   rounded float32 multiply, then one rounded float32 add (never an fma).  next_value float32 [rows] may be NULL.
 * gvec_categorical_target: logits_eval, logits_select float32 [rows][A][N], atoms innermost, finite at the legal actions;
 *   logits_select NULL = logits_eval.  N = num_atoms in [2, 64], support z_j = v_min + j * D, D = (v_max - v_min) / (N - 1).
 *   For i in S: p_i = softmax(logits_select[i]), Q_i = sum_j p_ij z_j;  a* = argmax_S Q_i;  p* = softmax(logits_eval[a*]).
 *   Tz_j = clamp(reward + discount * z_j, v_min, v_max), b_j = (Tz_j - v_min) / D, m_k = sum_j p*_j max(0, 1 - |b_j - k|),
 *   summed in ascending j: the gather form of the C51 projection, no atomics.  done[r] != 0 or nothing won: m is the projected
 *   point mass at clamp(reward, v_min, v_max), and no logits of a done row are read: its next_action is -1.
 *   m float32 [rows][N], next_action int64 [rows].  float32 throughout.
 * GVEC_E_INVALID (with a gvec_last_error message) before anything touches a device: args or a required pointer NULL (all but
 *   q_select / logits_select, discount and next_value), rows < 0 or rows >= 2^31, width or height outside [1, GVEC_MAX_DIM],
 *   obs_row_stride < 9*width*height, reserved != 0, num_atoms outside [2, 64], v_min or v_max not finite or v_min >= v_max.
 *   rows == 0 is a no-op that needs no device. */
typedef struct gvec_obs_valid_mask_args {
  int64_t rows;
  int32_t width, height;
  int64_t obs_row_stride;                                                                  /* floats, >= 9*width*height */
  const float* obs; uint8_t* mask;
} gvec_obs_valid_mask_args;
typedef struct gvec_q_target_args {
  int64_t rows;
  int32_t width, height;
  int64_t obs_row_stride;
  float gamma; int32_t reserved;
  const float* next_obs; const float* q_eval;
  const float* q_select;                                                                   /* NULL: q_eval */
  const float* reward;
  const float* discount;                                                                   /* NULL: gamma */
  const uint8_t* done;
  float* target; int64_t* next_action;
  float* next_value;                                                                       /* NULL: not wanted */
} gvec_q_target_args;
typedef struct gvec_categorical_target_args {
  int64_t rows;
  int32_t width, height;
  int64_t obs_row_stride;
  int32_t num_atoms; float gamma, v_min, v_max;
  const float* next_obs; const float* logits_eval;
  const float* logits_select;                                                              /* NULL: logits_eval */
  const float* reward;
  const float* discount;                                                                   /* NULL: gamma */
  const uint8_t* done;
  float* m; int64_t* next_action;
} gvec_categorical_target_args;
int32_t gvec_obs_valid_mask(int32_t device, void* hip_stream, const gvec_obs_valid_mask_args* args);
int32_t gvec_q_target(int32_t device, void* hip_stream, const gvec_q_target_args* args);
int32_t gvec_categorical_target(int32_t device, void* hip_stream, const gvec_categorical_target_args* args);

/* ---- board symmetries (D4), one per row: observations, masks, action-indexed values and actions -------
 * The rules of the game do not know left from right, so a stored transition is worth up to eight.  Handle-free like the feature
 * planes: DEVICE pointers on `device`, enqueued on hip_stream, nothing synchronises.  One launch moves every tensor of a row
 * with that row's symmetry.  Tile t = y*W + x, A = 5*H*W, action 5*t + d with d = up (0,-1), right (1,0), down (0,1),
 * left (-1,0), then 4 = the half move.
 * The group.  sym in [0, 8): fx = sym & 1, fy = sym & 2, tr = sym & 4.  g maps a source tile (x, y): if fx, x = W-1-x; if fy,
 *   y = H-1-y; then, if tr, x and y are swapped.  tr needs W == H: on another board only sym < 4 exists.  Direction vectors go
 *   through the same three steps, which permutes d -> d' (4 -> 4 always):
 *     sym 0 [0,1,2,3]  1 [0,3,2,1]  2 [2,1,0,3]  3 [2,3,0,1]  4 [3,2,1,0]  5 [3,0,1,2]  6 [1,2,3,0]  7 [1,0,3,2]
 *   Every sym is its own inverse except 5 and 6, which are each other's.
 * What a row's symmetry g does: a plane, out[g(t)] = in[t]; an action-indexed row (mask, values), out[5*g(t) + d'] =
 *   in[5*t + d]; an action a in [0, A), 5*g(a / 5) + d'(a % 5).  An action outside [0, A) is copied unchanged (-1 is what
 *   gvec_q_target returns for a row without a legal action).  Values are moved as bits: NaN payloads and -0.0 survive.
 * The half move.  Action 5*t + 4 names no direction: GeneralsEnv plays the first of up, right, down, left whose target is on
 *   the board (left when none is: a 1x1 board), d0(t).  That rule is not symmetric, so a half move from t is EXACT under g iff
 *   d0(g(t)) == d'(d0(t)): the move played from g(t) is the image of the move played from t.  When action_in is given, a row
 *   whose action is a half move in [0, A) that is not exact under its sym is transformed with the identity instead, every tensor
 *   of the row.  Full moves, out-of-range actions and calls without action_in restrict nothing.
 * sym uint8 [rows], required.  A value >= 8, or >= 4 where W != H, cannot be seen by the host: the row is transformed with the
 *   identity.  applied uint8 [rows], optional: the symmetry the row was transformed with (0 for a half move that fell back and
 *   for a sym out of range).
 * inverse != 0 transforms with the inverse of each row's symmetry.  The half-move rule is evaluated as in the forward call all
 *   the same - for sym itself, on action_in as given - so a call with inverse = 1, the same sym and the ORIGINAL action undoes
 *   exactly what the forward call did to the planes, the mask and the values (applied is the same in both).  action_out of
 *   such a call is the inverse image of the original action, which nobody needs; the forward call's action_out goes back
 *   through a FORWARD call whose sym is the inverse of its applied (a half move that was exact one way is exact back).
 * Plane sets: num_sets in [0, GVEC_SYM_MAX_PLANE_SETS]; set k reads in float32 [rows][planes][H*W], consecutive rows
 *   in_row_stride floats apart, and writes out float32 [rows][planes][H*W], dense.  mask_in -> mask_out uint8 [rows][A];
 *   values_in -> values_out float32 [rows][A]; action_in -> action_out int64 [rows].  Each pair is optional and goes together.
 *   EVERY element of every output is written.  No output may overlap any input.
 * GVEC_E_INVALID (with a gvec_last_error message) before anything touches a device: args or sym NULL, one half of a pair NULL,
 *   in or out of a set NULL, nothing to transform, num_sets outside [0, 4], planes outside [1, 64], in_row_stride <
 *   planes*width*height, rows < 0 or rows >= 2^31, width or height outside [1, GVEC_MAX_DIM], inverse outside {0, 1},
 *   reserved != 0, an output overlapping an input.  rows == 0 is a no-op that needs no device. */
#define GVEC_SYM_MAX_PLANE_SETS 4
typedef struct gvec_sym_plane_set {
  const float* in; float* out;
  int32_t planes;                                                                          /* 1 .. 64 */
  int64_t in_row_stride;                                                                   /* floats, >= planes*width*height */
} gvec_sym_plane_set;
typedef struct gvec_obs_symmetry_args {
  int64_t rows;
  int32_t width, height, num_sets, inverse, reserved;
  gvec_sym_plane_set sets[GVEC_SYM_MAX_PLANE_SETS];
  const uint8_t* sym;
  const uint8_t* mask_in; uint8_t* mask_out;                                               /* NULL: no mask */
  const float* values_in; float* values_out;                                               /* NULL: no values */
  const int64_t* action_in; int64_t* action_out;                                           /* NULL: no action, no half-move rule */
  uint8_t* applied;                                                                        /* NULL: not wanted */
} gvec_obs_symmetry_args;
int32_t gvec_obs_symmetry(int32_t device, void* hip_stream, const gvec_obs_symmetry_args* args);

/* ---- match arena: per-env episode tally and pairwise placements -------------------------------------------
 * Counts finished games where a self-play step's outputs already lie: one launch per env step, handle-free like the feature
 * planes (DEVICE pointers on `device`, enqueued on hip_stream, nothing synchronises).  All state is per env and owned by the
 * caller, so no atomic is needed and every number is the same from run to run.  rows = B envs, L = num_learners columns.
 * Inputs of the step: alive uint8 [B][L] (NULL: nobody is ever recorded as eliminated), terminated, truncated uint8 [B], reset
 *   uint8 [B] (this step re-dealt the env and played no turn; NULL: none did), winner int8 [B] (a player id or -1), reward
 *   float64 [B][L], player_ids int32 [L] (column -> player id), obs float32 [B][L][9][H*W] or NULL, consecutive observations
 *   obs_row_stride floats apart (only plane 1 is read, and only where an env is truncated).
 * Running state: death int32 [B][L] (0 alive, else the 1-based episode step at which the column was first seen not alive),
 *   ep_len int32 [B], ep_return float64 [B][L].  Totals: games int32 [B], wins, eliminated int32 [B][L], len_sum int64 [B],
 *   ret_sum float64 [B][L], pair2 int32 [B][L][L] (twice the score of column i against column j; the diagonal stays 0).
 * Per env b, in this order:
 *   1. reset[b] != 0: the running state is cleared (zeros) and nothing else happens.
 *   2. ep_len += 1; per column ep_return += reward, and death = ep_len where death == 0 and alive == 0.
 *   3. terminated[b] | truncated[b] != 0, the episode ends.  With games_cap > 0 and games[b] == games_cap nothing is counted.
 *      Otherwise a column's key is death when death != 0 (later is better) and 2^20 + land when it survived, land = the number
 *      of tiles with obs plane 1 == 0.5 (its own) when obs is given and the env was truncated without terminating, else 0; an
 *      episode is assumed shorter than 2^20 steps.  For i != j: pair2[i][j] += 2 where key_i > key_j, 1 where they are equal.
 *      games += 1, len_sum += ep_len, wins += (winner[b] == player_ids[column]), eliminated += (death != 0), ret_sum +=
 *      ep_return.  Counted or not, the running state is cleared.
 * Integer adds and plain float64 adds in this order: the result is defined to the bit.
 * GVEC_E_INVALID (with a gvec_last_error message) before anything touches a device: args or a required pointer NULL (all but
 *   alive, reset and obs), rows < 0 or rows >= 2^31, num_learners outside [1, GVEC_MAX_PLAYERS], games_cap < 0, and with obs:
 *   width or height outside [1, GVEC_MAX_DIM], obs_row_stride < 9*width*height.  rows == 0 is a no-op that needs no device. */
typedef struct gvec_arena_args {
  int64_t rows;
  int32_t width, height;                                                                   /* read with obs only */
  int32_t num_learners, games_cap;                                                         /* games_cap 0: no cap */
  int64_t obs_row_stride;                                                                  /* floats, >= 9*width*height */
  const uint8_t* alive;                                                                    /* NULL: everybody, always */
  const uint8_t* terminated; const uint8_t* truncated;
  const uint8_t* reset;                                                                    /* NULL: no env was re-dealt */
  const int8_t* winner; const double* reward; const int32_t* player_ids;
  const float* obs;                                                                        /* NULL: survivors tie */
  int32_t* death; int32_t* ep_len; double* ep_return;
  int32_t* games; int32_t* wins; int32_t* eliminated; int64_t* len_sum; double* ret_sum; int32_t* pair2;
} gvec_arena_args;
int32_t gvec_arena_update(int32_t device, void* hip_stream, const gvec_arena_args* args);

/* ---- experience gather support ---------------------------------------
 * Writes the compact state records of envs [env_begin, env_begin+n) into a device
 * buffer (e.g. a torch tensor handed to RCCL) as a slab [n] headers | [n] plane blocks |
 * [n] int32 army blocks: gvec_state_bytes_per_env() bytes per env.  Armies are always
 * int32 in a record, whatever form the env is stored in.  gvec_import_records checks
 * every record header against the handle's limits (board size, player count, reciprocal)
 * on the device and fails with GVEC_E_BOARD - that env left untouched - on a mismatch. */
int32_t gvec_export_records(gvec_handle* h, int32_t env_begin, int32_t n,
                            void* dst_device);
int32_t gvec_import_records(gvec_handle* h, int32_t env_begin, int32_t n,
                            const void* src_device);
/* Env dst_ids[i] of dst becomes exactly what env src_ids[i] of src is, for i < n: on-device clone / save / restore of env
 * states (search fan-out, checkpoints, rewinds) by one gather/scatter launch over the resident blocks.
 *   - src == NULL means src = dst.  dst_ids / src_ids are DEVICE int32 arrays on the handles' device; NULL = 0..n-1.
 *   - n == 0 is a no-op; n < 0 or dst == NULL: GVEC_E_INVALID.
 *   - Both handles must be plain (a sharded handle: GVEC_E_INVALID - copy between gvec_shard children; no call moves board
 *     state between devices), on the same device, with the same max_width, max_height, max_players and the same four
 *     production constants (prod_general, prod_city, prod_normal, normal_growth_interval).  Otherwise GVEC_E_INVALID, a
 *     gvec_last_error message naming the field, and nothing is launched.
 *   - Copied per pair: the header except the slot's lifetime counters (H_CNT_*: gvec_counters keeps counting the turns
 *     played in THIS handle), the whole planes block, the armies in the source's form, the gym reward baseline row
 *     (zeros when src never made one; allocated in dst when src has one and dst not) and the experience snapshot row
 *     (same rule).  Afterwards every call on dst behaves as if env dst_ids[i] had always held the state.  Draws keyed by
 *     env index stay keyed by the DESTINATION index (the on-device agent, the board pool's re-deal).
 *   - A pair naming an env outside [0, num_envs) of its handle is skipped and the call returns GVEC_E_RANGE (checked on
 *     the device, like gvec_import_records).
 *   - src_ids may repeat (fan-out); dst_ids must be distinct; with src == dst no env may be both a source and a destination
 *     of one call.  Neither is checked: the result is undefined otherwise.
 *   - Enqueued on dst's stream, after the work already enqueued on src's stream; src's stream then waits for the copy, so
 *     src's next call cannot overwrite a source mid-copy.  Synchronises dst's stream (the range check). */
int32_t gvec_copy_envs(gvec_handle* dst, const int32_t* dst_ids, gvec_handle* src, const int32_t* src_ids, int32_t n);
/* Zero-copy access for device consumers (torch-ROCm): the handle's resident device
 * arrays.  which: 0 header [B][24] u32, 1 bit-planes (the OwnedTiles planes at the end of an env's block are
 * meaningful only while its header flag bit 7 is set; otherwise the lists are the ownership planes - DESIGN.md
 * section 3), 2 armies (narrow form: u16, two 64-tile slots
 * interleaved per dword; authoritative for every env whose header flag bit 2 is clear - see
 * DESIGN.md section 3), 6 armies (wide form: int32, authoritative for the flagged envs), 3 legal masks
 * [B][max_players][mask_bytes], 4 actions [B][max_players], 5 err [B].  Consumers that want plain
 * per-tile planes use gvec_read_state with GVEC_MEM_DEVICE instead. */
#define GVEC_BUF_HEADER  0
#define GVEC_BUF_ROWS    1
#define GVEC_BUF_ARMY    2
#define GVEC_BUF_LEGAL   3
#define GVEC_BUF_ACTIONS 4
#define GVEC_BUF_ERR     5
#define GVEC_BUF_ARMY_WIDE 6
void*   gvec_device_buffer(gvec_handle* h, int32_t which);
/* A byte range of one of the handle's small per-env buffers - GVEC_BUF_HEADER, _LEGAL, _ACTIONS (what the device agent
 * played, while gvec_record_agent_actions is on) or _ERR (the per-env codes of the last gvec_step in host mode or, while
 * recording is on, of the last per-turn gvec_rollout launch) - copied to host memory; synchronises the handle's stream. */
int32_t gvec_read_buffer(gvec_handle* h, int32_t which, uint64_t byte_offset, uint64_t bytes, void* host_dst);

/* Runs the on-device self-test of the wave primitives (DPP shifts, scans,
 * bpermute); 0 = pass.  Used by smoke tests on new driver / hardware revisions. */
int32_t gvec_selftest(int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* GENERALS_VEC_H */
