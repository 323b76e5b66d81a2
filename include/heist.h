/* heist.h -- C ABI of the MI355X-native Heist Architect hot path (libheist_hip.so).
 *
 * The reference (a pure-Python package) has no FFI for this path; its boundary is the
 * Python class API that training and the UI call.  Each entry point below replaces one
 * reference interface (paths relative to the reference repository root) and is bound
 * by the Python mirror package heist_amd (see INTEGRATION.md for the ctypes binding).
 *
 * Conventions
 *  - All array pointers are DEVICE pointers owned by the caller (e.g. torch tensors on
 *    the same HIP device), except `reward_consts` in heist_create (host).
 *  - Every call is enqueued on `stream` and is asynchronous; nothing synchronises.
 *  - Return 0 on success, HEIST_EINVAL for bad arguments, else a hipError_t value.
 *    heist_last_error() gives a message for the calling thread's last failure.
 *  - A heist_t handle is bound to the device that was current at heist_create and is
 *    not thread-safe: use one handle per device/thread.
 *  - Layouts are [env][...] row-major; grids are [env][row][col]; obs is [env][3][R][C].
 */
#ifndef HEIST_H
#define HEIST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: heist_step_stamps takes the buffer size; heist_stamp_words; 3: heist_arch_update_*;
 * 4: heist_arch_update_status, the heist_*_nhwc training passes, heist_get_config's 15th word
 *    (heist_step on the lean kernel), the heist_train_* fp32-MFMA training convolutions,
 *    heist_rollout_tally; 5: heist_get_config's 16th word (lean_waves), heist_lstm_cell */
#define HEIST_ABI_VERSION 5
#define HEIST_EINVAL 100000

/* status_out codes of heist_step (environment.py:236-297 info["status"]). */
#define HEIST_RUNNING 0
#define HEIST_DETECTED 1
#define HEIST_VAULT_REACHED 2
#define HEIST_TIMEOUT 3
#define HEIST_ALREADY_DONE 4

typedef struct heist_env* heist_t;
typedef struct ihipStream_t* heist_stream_t; /* == hipStream_t */

int heist_abi_version(void);
const char* heist_last_error(void);

/* Replaces HeistEnvironment.__init__ / EnvironmentConfig (environment.py:18-97) for a
 * batch of n_envs independent environments (1 <= n_envs <= 2^24).  R, C <= 64.  reward_consts (host) =
 * {reward_step, reward_detection, reward_vault}.  max_cams / max_guards / max_path bound
 * the per-env layout capacity. */
int heist_create(int rows, int cols, int max_steps, int start_r, int start_c, int vault_r, int vault_c,
                 const double* reward_consts, int n_envs, int max_cams, int max_guards, int max_path,
                 heist_t* out);
int heist_destroy(heist_t h);

/* Replaces HeistEnvironment.set_layout + _reset_layout + is_level_valid
 * (environment.py:102-177) and BudgetManager.purchase (budget.py:48-58), per env:
 *   wall_rc     [N][max_walls][2]      int32   walls in list order (first n_walls[e] used)
 *   cam_params  [N][max_cams][6]       float64 row, col, fov_angle, heading, rotation_speed, vision_range
 *   guard_paths [N][max_guards][max_path][2] int32 patrol_path points
 *   guard_meta  [N][max_guards][3]     int32   path length, speed, vision_range
 *   guard_fov   [N][max_guards]        float64 fov_angle
 *   budget      [N]                    int32   BudgetManager.total_budget
 *   mask        [N]                    uint8   only envs with mask[e] != 0 are re-laid out (NULL: all)
 *   valid_out   [N]                    uint8   bfs_path_exists(start, vault) (written for masked envs)
 * Guard path points must lie inside the grid.  Solver state is left untouched (call
 * heist_reset next, as training.py:516 does). */
int heist_set_layout(heist_t h, int max_walls, const int32_t* wall_rc, const int32_t* n_walls,
                     const double* cam_params, const int32_t* n_cams, const int32_t* guard_paths,
                     const int32_t* guard_meta, const double* guard_fov, const int32_t* n_guards,
                     const int32_t* budget, const uint8_t* mask, uint8_t* valid_out, heist_stream_t stream);

/* Replaces HeistEnvironment.reset + get_state_tensor (environment.py:183-214, :347-374)
 * for envs with mask[e] != 0 (mask == NULL: all).  obs_out [N][3][R][C] float32; rows of
 * unmasked envs are not written. */
int heist_reset(heist_t h, const uint8_t* mask, float* obs_out, heist_stream_t stream);

/* Replaces HeistEnvironment.step + get_state_tensor (environment.py:216-299, :347-374).
 *   actions [N] int64 in 0..4;  obs_out [N][3][R][C] float32;  reward_out [N] float32
 *   (the float64 reward rounded, as agents/solver.py:138 stores it); reward64_out [N]
 *   float64 or NULL; done_out [N] uint8; status_out [N] int8 (HEIST_* codes).
 * With HEIST_STEP_LEAN=1 at heist_create, where the lean K-tick kernel serves the handle
 * (20 x 20 at one wave per env, 32 x 32; no instrumentation armed) the tick runs as
 * heist_step_multi with K = 1, bit-identical (off by default: slower per tick).
 * auto_reset != 0: an env that finishes this tick is reset in the same launch and its
 * obs row holds the reset observation (training.py:515-520 next attempt), while reward,
 * done and status describe the finishing tick.  auto_reset == 0: finished envs answer
 * later steps with reward 0 / HEIST_ALREADY_DONE (environment.py:232-233). */
int heist_step(heist_t h, const int64_t* actions, float* obs_out, float* reward_out, double* reward64_out,
               uint8_t* done_out, int8_t* status_out, int auto_reset, heist_stream_t stream);

/* K consecutive heist_step calls in one launch, for actions known in advance (env-only
 * throughput, action replay; no reference counterpart as an entry point -- it is
 * environment.py:216-299 + :347-374 applied K times).  Equivalent, bit for bit, to
 *   for k in 0..K-1: heist_step(h, actions + k*N, obs_out + k*N*3*R*C, reward_out + k*N,
 *                               reward64_out ? reward64_out + k*N : NULL, done_out + k*N,
 *                               status_out + k*N, auto_reset, stream)
 * with every per-tick output written (tick-major: actions [K][N] int64, obs_out
 * [K][N][3][R][C] float32, reward_out [K][N] float32, reward64_out [K][N] float64 or NULL,
 * done_out [K][N] uint8, status_out [K][N] int8); the per-env state stays on chip between
 * the ticks.  1 <= K <= 1024.  Launches read a table of the shared camera fan that a launch
 * refills when it is stale; a launch on another stream than the previous one refills it
 * after waiting, on the device, for that launch (no host synchronisation). */
int heist_step_multi(heist_t h, int K, const int64_t* actions, float* obs_out, float* reward_out,
                     double* reward64_out, uint8_t* done_out, int8_t* status_out, int auto_reset,
                     heist_stream_t stream);

/* Copies per-env state out for get_environment_state / the single-env compatibility
 * class (environment.py:388-417).  Any pointer may be NULL.
 *   scalars [N][12] int32: pos_r, pos_c, tick, done, detected, vault_reached, prev_dist,
 *                          initial_dist, n_cams, n_guards, n_walls, budget_spent
 *   grid [N][R][C] int8;  cam_heading [N][max_cams] f64;  guard_idx [N][max_guards] int32;
 *   guard_heading [N][max_guards] f64 */
int heist_export(heist_t h, int32_t* scalars, int8_t* grid, double* cam_heading, int32_t* guard_idx,
                 double* guard_heading, heist_stream_t stream);

/* Env state blobs, no reference counterpart as an entry point: a restatement of everything
 * HeistEnvironment.reset / step read and write (environment.py:183-299: solver_pos, tick, done,
 * solver_detected, vault_reached, _prev_dist, _initial_dist, every camera's heading, every guard's
 * current_idx and heading) together with the layout they run on (environment.py:102-152: grid,
 * cameras, guards and their patrol paths, the budget spent), so that a saved env can be put back,
 * moved to another handle or process, or forked.
 * After heist_state_load every later heist_step, heist_step_multi, heist_reset, heist_export,
 * heist_obs_pack of its rows and heist_set_layout on a loaded env gives, bit for bit, what the
 * saved env would have given from the moment of heist_state_save -- on the same handle after its
 * layouts changed, on another handle, in another process -- provided the handle was created with
 * the same heist_create arguments (n_envs apart) and the same guard-cone setting.  Knobs that do
 * not change results may differ (HEIST_STEP_WAVES, HEIST_LEAN, HEIST_LEAN_WAVES, HEIST_STEP_LEAN,
 * the ray mode).  Sample counters and stamps are instrumentation, not state: not saved.
 * One blob is heist_state_bytes(h) bytes, a multiple of 16 and a function of rows, cols, max_cams,
 * max_guards, max_path, the guard-cone setting and the format version (944 B at 20 x 20 with
 * max_cams 5, max_guards 3, max_path 8; 1,696 B at 32 x 32 with the same; -1 on a bad handle):
 *   64 B   header: 16 little-endian uint32 = magic 0x54534548, format version 1, rows, cols,
 *          max_cams, max_guards, max_path, guard_cones, max_steps, start r, c, vault r, c, 0, 0, 0
 *   48 B   the 12 int32 scalars of heist_export
 *   32 B x max_cams    fov, heading, speed (float64), row, col, range, rays (int16)
 *   32 B x max_guards  fov, heading (float64), patrol index, step, length, range, rays (int16),
 *                      position, patrol start (uint16 r | c << 8), two cone-cache slots (uint8)
 *   2 B x max_guards x max_path patrol points (r | c << 8), padded to 16 B
 *   rows x cols B      grid (int8 tiles), padded to 16 B
 *   the bit-packed raycast stop map of the grid with its 6-cell border, padded to 16 B
 * The guard cone cache (8 KB per guard) is not in the blob: a load rebuilds it with the kernel
 * heist_set_layout uses, recomputes the dispatch order and marks the K-tick fan table stale, as
 * heist_set_layout does.
 * heist_state_save: blobs [m][bytes] (16-byte aligned), blob i = env env_ids[i] (int32, device;
 *   NULL: envs 0..m-1).  Reads the env only.  An env id outside [0, n_envs) gives a blob of zeros,
 *   which no load accepts.
 * heist_state_load: env env_ids[i] (NULL: i) <- blob blob_index[i] (int32, device; NULL: i) of
 *   blobs [n_blobs][bytes]; a fork is blob_index naming one blob many times.  status_out [m] uint8
 *   (may be NULL): 1 loaded, 0 rejected with the env left untouched -- an env id outside
 *   [0, n_envs), an env named by more than one item (all of them are rejected), a blob index
 *   outside [0, n_blobs), a header that differs from the handle's in any word, or records that do
 *   not fit the handle's capacities.  blobs must stay unchanged until the call's work on `stream`
 *   is done.  Two loads on one handle must not run concurrently on different streams (they share
 *   the handle's scratch).
 * HEIST_EINVAL: m < 0, n_blobs < 0, blobs NULL with m > 0, blobs not 16-byte aligned, a save of
 * m > n_envs without env_ids.  m == 0 is a no-op. */
int64_t heist_state_bytes(heist_t h);
int heist_state_save(heist_t h, const int32_t* env_ids, int m, void* blobs, heist_stream_t stream);
int heist_state_load(heist_t h, const int32_t* env_ids, int m, const void* blobs, int n_blobs,
                     const int32_t* blob_index, uint8_t* status_out, heist_stream_t stream);

/* Fork inside a handle, no reference counterpart: item i makes env dst_ids[i] equal to env
 * src_ids[i] of the same handle (both int32 [m], device, required; a source may be named many
 * times: one root, many children).  One launch, no blob, no rebuild, no scratch.
 * After the call every later heist_step, heist_step_multi, heist_step_multi_records, heist_reset,
 * heist_export, heist_plan, heist_state_save and heist_set_layout on dst gives, bit for bit, what
 * the same call gives on src from this moment: heist_state_load's contract without the blob.
 * An accepted item copies what a blob holds for the env -- scalars, every camera and guard record
 * as it stands, paths, grid, stop map -- and the guard cone cache: for each live guard the source
 * has cached, its cone block (the rows of its patrol points: every entry a later call can read)
 * is copied from src, or kept where dst already held it.  It is kept
 * exactly when, before the call, dst's guard of that index was live and cached and dst's grid,
 * the guard's fov, step, length, range, rays and patrol start and its patrol points equalled
 * src's (the block is a function of those: the usual case when the children of one root are
 * forked again every few ticks).
 *   status_out [m] uint8 (may be NULL):
 *     0 rejected, dst untouched: an id outside [0, n_envs), src == dst, a dst that another item
 *       names as dst (every such item is rejected) or that any item names as src
 *     1 forked; every cached guard's cones copied, or the source has no cached guard
 *     2 forked; every cached guard's cones kept
 *     3 forked; some cones kept and some copied
 * So sources are only read during the launch and every destination has one writer.  Like
 * heist_state_load it recomputes the dispatch order and marks the K-tick fan table stale.  Two
 * forks, or a fork and a load, on one handle must not run concurrently on different streams (a
 * fork reads envs the other may be writing, and both rewrite the dispatch order).
 * HEIST_EINVAL: m < 0, a NULL src_ids or dst_ids with m > 0.  m == 0 is a no-op. */
int heist_state_fork(heist_t h, const int32_t* src_ids, const int32_t* dst_ids, int m, uint8_t* status_out,
                     heist_stream_t stream);

/* Compact observation records, no reference counterpart as an entry point: a lossless restatement
 * of get_state_tensor's output (environment.py:305-374) for callers that keep many observations
 * (the trainer's rollout buffer).  Channel 0 is grid / 5 and constant while a layout stands, channel
 * 2 is a function of the vault's and the solver's cell, and channel 1 is one bit per cell, so a
 * record holds the bits and the cell; the grid is kept once per env.
 * One record is W little-endian uint32 words, W = ceil(R*C / 32) + 1 rounded up to a multiple of 4
 * (16-byte records): 64 B at 20 x 20, 144 B at 32 x 32, 32 B at 13 x 17 and 10 x 10, 528 B at 64 x 64.
 *   words 0 .. ceil(R*C/32)-1: visibility; bit i of word j is cell 32 j + i (row-major, r*C + c),
 *     1 iff channel 1 of the cell is non-zero; bits past R*C are 0
 *   the next word: pos_r | pos_c << 8, the solver's cell
 *   the remaining words: 0 (equal observations give byte-equal records)
 * heist_obs_record_bytes: 4 W, or -1 (heist_last_error) unless 1 <= rows, cols <= 64.
 * heist_obs_pack: obs [n][3][R][C] float32 (heist_reset / heist_step output, or the [K][N] rows of
 *   a heist_step_multi launch) -> records [n][W].  The solver's cell is the one cell of channel 2
 *   above 0.5 (1 - 0.3 d / (R + C) >= 0.7 there, every other cell <= 0); with no such cell the solver
 *   stands on the vault, whose -1 overwrites its 1 (environment.py:359-360), and the record holds
 *   (vault_r, vault_c).
 * heist_obs_expand: obs_out [m][3][R][C] float32, sample i rebuilt from record j = index[i] (int64;
 *   index == NULL: j = i) of records [n_records][W], bit-identical to the observation the record was
 *   packed from: channel 0 = (float)grid[rec_env[j]][cell] / 5.0f with grid [n_envs][R][C] int8 as
 *   heist_export wrote it while the records' layouts stood, channel 1 = bit ? 1.0f : 0.0f, channel
 *   2 = base + (float)(-0.3 * ((double)d / (double)(R + C))) with base -1 on the vault, else 1 on the
 *   solver's cell, else 0, and d the Manhattan distance to the vault (environment.py:357-367).
 *   rec_env [n_records] int32 is each record's env.  It takes no handle: records and the grid
 *   snapshot stay valid after heist_set_layout changes the env.  A j outside [0, n_records) or an
 *   env outside [0, n_envs) gives a sample of NaNs.
 * n, m >= 0 (0: no-op).  16-byte aligned obs / obs_out with R*C a multiple of 4 take the 16-byte
 * load / store path. */
int heist_obs_record_bytes(int rows, int cols);
int heist_obs_pack(const float* obs, int64_t n, int rows, int cols, int vault_r, int vault_c, uint32_t* records,
                   heist_stream_t stream);
int heist_obs_expand(const uint32_t* records, int64_t n_records, const int32_t* rec_env, const int64_t* index, int64_t m,
                     const int8_t* grid, int n_envs, int rows, int cols, int vault_r, int vault_c, float* obs_out,
                     heist_stream_t stream);

/* heist_step_multi with the compact record of every row in place of the row itself, no reference
 * counterpart as an entry point (action replay, search from forked states, offline datasets: K
 * ticks of N envs are K N records, 64 B each at 20 x 20, instead of K N rows of 4,800 B).
 *   records_out [K][N][W] uint32, W = heist_obs_record_bytes(rows, cols) / 4, 16-byte aligned:
 *   records_out[k][e] equals, byte for byte, what heist_obs_pack gives for row [k][e] of the
 *   heist_step_multi launch with the same arguments; reward_out, reward64_out, done_out and
 *   status_out are bit-identical to that launch's and the handle ends in the same state.
 * heist_step_records_direct: 1 when the K-tick kernel writes the records itself (the lean or the
 *   generic K-tick kernel serves the handle and no stamps are armed: no observation row is
 *   written anywhere and obs_scratch is not touched), 0 when the fallback runs, -1 on a bad handle.
 * Fallback (no K-tick kernel for the grid, e.g. cols not a multiple of 4, or sample counters,
 *   stamps or a probe mode armed): K times heist_step into obs_scratch [N][3][R][C] float32 and
 *   heist_obs_pack of it, on `stream`; obs_scratch may be NULL only on the direct route.
 * HEIST_EINVAL: K outside 1..1024, a NULL actions, records_out, reward_out, done_out or
 * status_out, records_out not 16-byte aligned, obs_scratch NULL when the fallback is needed. */
int heist_step_records_direct(heist_t h);
int heist_step_multi_records(heist_t h, int K, const int64_t* actions, uint32_t* records_out, float* reward_out,
                             double* reward64_out, uint8_t* done_out, int8_t* status_out, int auto_reset,
                             float* obs_scratch, heist_stream_t stream);

/* Exact Solver planner, no reference counterpart: for every env in its current state, the fewest
 * ticks in which some action sequence fed to heist_step_multi(..., auto_reset = 0) ends a tick with
 * vault_reached == 1 and detected == 0, and one such sequence.  Cameras and guards move on a
 * schedule the Solver does not influence (environment.py:250-258), so with
 *   reach_0 = {the solver's cell} (empty for an env already done),
 *   cand_k  = (reach_{k-1} and its four one-cell shifts inside the grid) minus wall cells,
 *   vis_k   = the visibility plane heist_step would compute on the env's k-th tick from now,
 * T is the first k >= 1 with vault in cand_k \ vis_k, and reach_k = cand_k \ vis_k \ {vault}, empty
 * once tick + k >= max_steps (the arrival on the tick that times out still counts).  Env e plans
 * min(horizon, max_steps - tick[e]) ticks.
 *   ticks_out   [N] int32: T, or -1 when no k within those ticks qualifies (env done, no path,
 *               the vault always seen on arrival, max_steps first, horizon too short).
 *   actions_out [horizon][N] int64, heist_step_multi's `actions` as it stands: rows 0 .. T-1 hold
 *               the canonical plan -- from x_T = vault, a_k is the lowest action (0 WAIT, 1 UP, 2
 *               DOWN, 3 LEFT, 4 RIGHT) with x_k - delta(a_k) in reach_{k-1}, that cell being
 *               x_{k-1} -- and every other entry is 0.
 *   reach_out   [horizon][N][W] uint32, W = heist_obs_record_bytes(rows, cols) / 4, 16-byte aligned,
 *               required (it is also the backtrack's history): row k-1 holds reach_k in the record's
 *               bit order (bit i of word j is cell 32 j + i), words past ceil(R*C/32) are 0, rows of
 *               ticks >= T and rows after the set empties are 0.
 * The launch only reads the env: state, shared-fan bookkeeping, counters and stamps are untouched
 * and a later launch gives, bit for bit, what it would have given without the call.
 * heist_plan_supported: 1 when a planner kernel exists for the handle's (K-tick waves, grid size
 *   class) -- every grid up to 64 x 64 at the default waves, cols need not be a multiple of 4 --
 *   else 0; -1 on a bad handle.
 * HEIST_EINVAL: horizon outside 1..1024, a NULL ticks_out, actions_out or reach_out, reach_out not
 * 16-byte aligned, a probe mode armed (HEIST_PROBE_MODE), heist_plan_supported 0. */
int heist_plan_supported(heist_t h);
int heist_plan(heist_t h, int horizon, int32_t* ticks_out, int64_t* actions_out, uint32_t* reach_out,
               heist_stream_t stream);

/* Planner field, no reference counterpart: heist_plan's answer for every cell of every env at once
 * -- the exact value function of the Solver's game against the emitters' schedule.  Env e runs
 * HK = min(horizon, max_steps - tick[e]) ticks, 0 for an env already done.  With
 *   vis_k      = heist_plan's vis_k, k = 1 .. HK,
 *   move(x, a) = x + delta(a) if that cell is inside the grid and not a wall tile, else x
 *                (0 WAIT, 1 UP, 2 DOWN, 3 LEFT, 4 RIGHT),
 *   togo_HK[x] = none for every cell,
 * and for k = HK-1 .. 0 and every non-wall cell x, the vault's included,
 *   togo_k[x]  = the minimum over the five actions a, y = move(x, a), of
 *                none                if y is in vis_{k+1},
 *                1                   if y is the vault,
 *                none                if togo_{k+1}[y] is none,
 *                togo_{k+1}[y] + 1   otherwise;
 * wall cells are none, and none is stored as -1.  togo_0[x] is what heist_plan returns as ticks_out
 * for this env with the Solver's cell set to x, the max_steps rule included (an arrival on the
 * tick that times out counts); every cell of a done env is -1.
 *   togo_out       [N][R*C] int16: togo_0, in 1 .. 1024 or -1.
 *   action_out     [N][R*C] int8: the lowest action that attains togo_0[x], -1 where togo_0[x] is -1.
 *   vis_out        [horizon][N][W] uint32, W = heist_obs_record_bytes(rows, cols) / 4, 16-byte
 *                  aligned, required (it is also the backward sweep's history): row k-1 holds vis_k
 *                  in the record's bit order (bit i of word j is cell 32 j + i), bits past R*C and
 *                  words past ceil(R*C/32) are 0, rows k >= HK are 0.
 *   togo_ticks_out [horizon][N][R*C] int16 or NULL, 2-byte aligned: row k holds togo_k for k < HK
 *                  (row 0 equals togo_out), rows k >= HK are -1.
 * The launch only reads the env, as heist_plan does: state, shared-fan bookkeeping, counters and
 * stamps are untouched.
 * heist_plan_field_supported: heist_plan_supported's value.
 * HEIST_EINVAL: horizon outside 1..1024, a NULL togo_out, action_out or vis_out, vis_out not
 * 16-byte aligned, a probe mode armed (HEIST_PROBE_MODE), heist_plan_field_supported 0. */
int heist_plan_field_supported(heist_t h);
int heist_plan_field(heist_t h, int horizon, int16_t* togo_out, int8_t* action_out, uint32_t* vis_out,
                     int16_t* togo_ticks_out, heist_stream_t stream);

/* Planner value, no reference counterpart: the exact optimal discounted return of the Solver from
 * every cell of every env -- heist_plan_field's recurrence under the env's own step reward
 * (environment.py:235, :261-297) instead of a tick count.  Env e runs HK = min(horizon,
 * max_steps - tick[e]) steps, 0 for an env already done.  With vis_k and move(x, a) as in
 * heist_plan_field, dist(x) the Manhattan distance from x to the vault, D0 the env's initial_dist,
 * r_step, r_detect, r_vault the handle's reward_consts, tick the env's tick and
 *   V_HK[x] = 0.0 for every cell,
 * for k = HK-1 .. 0, every non-wall cell x (the vault's included) and a = 0 .. 4 in order, with
 * y = move(x, a) and curr = dist(y), each line one IEEE double operation, none contracted:
 *   rew = r_step
 *   rew = rew + (double)(dist(x) - curr) * 0.1
 *   if curr <= 3 and D0 > 3:   rew = rew + 0.05 * (double)(3 - curr)
 *   seen = y in vis_{k+1};     if seen:       rew = rew + r_detect
 *                              if y == vault: rew = rew + r_vault          (both may apply)
 *   last = tick + k + 1 >= max_steps
 *   if last: frac = 1.0 - (double)curr / (double)max(D0, 1); if frac < 0: frac = 0;
 *            rew = rew + frac * 2.0
 *   q = (seen or y == vault or last) ? rew : rew + gamma * V_{k+1}[y]
 * V_k[x] is the maximum q under a strict greater-than (the first maximum stays: a blocked move
 * ties with WAIT and is never chosen) and the action is that first a.  Wall cells hold 0.0 and -1;
 * every cell of an env with HK = 0 holds 0.0 and -1.
 * V_0[pos] is the largest value, over the action sequences heist_step_multi(..., auto_reset = 0)
 * can be fed for HK ticks, of the reward64 of tick k times gamma^k summed from the back
 * (r_k + gamma * (...)), for an env whose prev_dist equals dist(pos): heist_reset and heist_step
 * always leave it so, only an edited state blob does not.  With horizon < max_steps - tick it is
 * the horizon-truncated return.
 *   value_out        [N][R*C] float64, 8-byte aligned: V_0.
 *   action_out       [N][R*C] int8: the action at k = 0.
 *   vis_out          [horizon][N][W] uint32, 16-byte aligned, required: exactly heist_plan_field's
 *                    vis_out, padding and rows k >= HK included.
 *   value_ticks_out  [horizon][N][R*C] float64 or NULL, 8-byte aligned: row k holds V_k for k < HK
 *                    (row 0 equals value_out), rows k >= HK are 0.0.
 *   action_ticks_out [horizon][N][R*C] int8 or NULL: row k holds the actions of step k, rows
 *                    k >= HK are -1.  The two optional outputs are independent of each other.
 * The launch only reads the env, as heist_plan_field does.
 * heist_plan_value_supported: 1 where heist_plan_field_supported is 1, one word per lane fetches a
 *   visibility row and the kernel's LDS -- heist_plan_field's plus 12 R C bytes: two float64
 *   [R*C] arrays -- fits the 64 KB a workgroup gets by default: every grid up to 32 x 32 at 1, 2 and
 *   4 K-tick waves.  The dynamic LDS limit is not raised: at 64 x 64 the two arrays alone are
 *   64 KB and the value is 0.  -1 on a bad handle.
 * HEIST_EINVAL: horizon outside 1..1024, gamma not finite or outside [0, 1], a NULL value_out,
 * action_out or vis_out, vis_out not 16-byte aligned, value_out or value_ticks_out not 8-byte
 * aligned, a probe mode armed (HEIST_PROBE_MODE), heist_plan_value_supported 0. */
int heist_plan_value_supported(heist_t h);
int heist_plan_value(heist_t h, int horizon, double gamma, double* value_out, int8_t* action_out,
                     uint32_t* vis_out, double* value_ticks_out, int8_t* action_ticks_out,
                     heist_stream_t stream);

/* Planner what-if, no reference counterpart: heist_plan_field's fewest ticks and heist_plan_value's
 * optimal return of every env with some of its emitters switched off -- M variants per env in one
 * launch, which is what tells which camera or guard a layout's difficulty comes from.  Visibility is
 * a union over the emitters, and an emitter blocks neither a ray nor a move (only wall tiles do), so
 * "slot j is off" is defined at any tick of any env: the slot's record still advances every tick
 * (camera heading, guard patrol index and heading), it casts no ray, stamps no cached cone and, for
 * a guard cast live, does not mark its own cell.  The grid stays as heist_set_layout left it: a
 * guard is placed without a placement check and its start tile replaces a wall under it, and a
 * switched-off guard does not put that wall back (a layout rebuilt without the guard would).
 *   emitter_mask [N][M] uint64, 8-byte aligned, M >= 1: bit j of emitter_mask[e][m] says slot j of
 *                env e is live in variant (e, m).  Slots are numbered as everywhere else: cameras
 *                0 .. max_cams-1, then guard g at max_cams + g.  Bits of slots the env does not fill
 *                (camera slots from n_cams[e] up, guard slots from n_guards[e] up) and bits at or
 *                above max_cams + max_guards are ignored.
 * Variant (e, m) is planned from env e's current state -- its tick, its emitters' poses, its
 * Solver's cell pos -- exactly as heist_plan_field and heist_plan_value plan it, HK = min(horizon,
 * max_steps - tick[e]) ticks (0 for an env already done), with vis_k the union over the live slots
 * alone; togo_0 and V_0 below are heist_plan_field's and heist_plan_value's recurrences over those
 * vis_k, V_0 in heist_plan_value's own arithmetic (the same lines in the same order, each one IEEE
 * double operation, none contracted, the first maximum under a strict greater-than).
 *   ticks_out       [N][M] int16: togo_0[pos], in 1 .. 1024 or -1 (no undetected way to the vault).
 *   value_out       [N][M] float64, 8-byte aligned: V_0[pos].
 *   action_out      [N][M] int8: heist_plan_value's action at pos and k = 0.
 *   vis_out         [horizon][N][M][W] uint32, W = heist_obs_record_bytes(rows, cols) / 4, 16-byte
 *                   aligned, required (it is the backward sweeps' history): row (k-1, e, m), at
 *                   (((k-1) N + e) M + m) W words, holds variant (e, m)'s vis_k in the record's bit
 *                   order, padding as in heist_plan_field, rows k > HK are 0.  For M = 1 this is
 *                   heist_plan_field's layout.
 *   togo_cells_out  [N][M][R*C] int16 or NULL: the whole togo_0 (wall cells -1).
 *   value_cells_out [N][M][R*C] float64 or NULL, 8-byte aligned: the whole V_0 (wall cells 0.0).
 *                   The two optional outputs are independent of each other; there are no per-tick
 *                   tables here.
 * Every variant of an env with HK = 0 holds -1 / 0.0 / -1, in the cell tables too.
 * A variant with every filled slot's bit set is heist_plan_field / heist_plan_value on the same
 * handle, bit for bit: ticks_out = togo_out[e][pos], value_out = value_out[e][pos], action_out =
 * heist_plan_value's action_out[e][pos], the cell tables their togo_out / value_out, the vis rows
 * their vis_out.  A variant with no bit set is the same pair of calls on the layout's walls alone.
 * The launch only reads the env, as heist_plan_field does.
 * heist_plan_masked_supported: heist_plan_value_supported's value -- the kernel's LDS is
 *   heist_plan_value's (the tick counts lie over one of the two float64 arrays): every grid up to
 *   32 x 32 at 1, 2 and 4 K-tick waves; 64 x 64 is not supported.  -1 on a bad handle.
 * HEIST_EINVAL: horizon outside 1..1024, gamma not finite or outside [0, 1], M < 1 or N M >= 2^31,
 * a NULL emitter_mask, ticks_out, value_out, action_out or vis_out, vis_out not 16-byte aligned,
 * emitter_mask, value_out or value_cells_out not 8-byte aligned, a probe mode armed
 * (HEIST_PROBE_MODE), heist_plan_masked_supported 0. */
int heist_plan_masked_supported(heist_t h);
int heist_plan_masked(heist_t h, int horizon, double gamma, int M, const uint64_t* emitter_mask,
                      int16_t* ticks_out, double* value_out, int8_t* action_out, uint32_t* vis_out,
                      int16_t* togo_cells_out, double* value_cells_out, heist_stream_t stream);

/* Planner placement, no reference counterpart: heist_plan_masked's two answers for every env with
 * one more camera in it -- M candidate cameras per env in one launch, which is what tells where a
 * camera the layout does not have would have mattered, and how much.  Visibility is a union over the
 * emitters, an emitter blocks neither a ray nor a move (only wall tiles do), and a camera is only
 * ever placed on an EMPTY tile (environment.py:124-135, :160-167), so it never changes the wall
 * plane: the visibility of "this layout plus camera X" on a tick is the layout's own row OR X's cone
 * on that tick.  The launch therefore casts the candidate alone, against the env's wall plane, and
 * takes the layout's share as given rows; none of the env's own emitters is read or cast.
 *   cand     [N][M][6] float64, 8-byte aligned, M >= 1: cand[e][m] is a heist_set_layout cam_params
 *            row (row, col, fov_angle, heading, rotation_speed, vision_range) and becomes a camera
 *            record by heist_set_layout's own conversion of an accepted camera: tile ((int)row,
 *            (int)col), range (int)vision_range, max(int(fov_angle * 2), 30) rays.  heading is the
 *            camera's heading now, at env e's current tick: planned tick k = 1 .. HK first rotates
 *            it, heading = (heading + rotation_speed * 1.0) mod 360 (Python's %, once per tick,
 *            accumulated as the env's cameras accumulate it), and then casts, as an env camera does.
 *   base_vis [horizon][N][W] uint32, W = heist_obs_record_bytes(rows, cols) / 4, 16-byte aligned:
 *            row (k-1, e) holds the visibility on tick k that the candidates are added to, in the
 *            record's bit order -- heist_plan_field's, heist_plan_value's or (M = 1) heist_plan_masked's
 *            vis_out of the same handle state.  It is trusted as given: its words 0 .. ceil(R C /
 *            32) - 1 of the rows k <= HK are used as they are, nothing else of it is read.  With
 *            heist_plan_field's rows the result is "the layout plus X"; with the rows of a
 *            heist_plan_masked variant that switches slot j off it is "the layout without slot j,
 *            plus X", a relocation.  base_vis and vis_out must not overlap.
 * Candidate (e, m) is valid iff both hold:
 *   1. it is placeable in env e's grid as it stands (environment.py:160-167): with r = (int)row, c =
 *      (int)col, 0 < r < R-1, 0 < c < C-1 and tile (r, c) is EMPTY -- not a wall, the start, the
 *      vault, a camera or a guard's start tile.  One divergence from a layout rebuilt with the
 *      candidate in its camera list: heist_set_layout places cameras before guards, so there a
 *      camera on a guard's start tile is accepted (the guard then takes the tile over); here it is
 *      not.  The budget and the camera slots are ignored, as if 3 points and a free slot were there;
 *   2. its parameters are ones the raycaster takes, every comparison false for a NaN:
 *        |row| < 2^31 and |col| < 2^31      (the (int) conversions are defined)
 *        0 < fov_angle <= 16000             (the ray count stops growing there; it fits the int16)
 *        |heading| <= 1e300, |rotation_speed| <= 1e300   (their sum is finite; every rotated
 *                                            heading then lies in [0, 360])
 *        0 <= vision_range < 32768          (the record's int16 range)
 *      No float64 bit pattern in cand makes the launch read or write out of bounds: a candidate
 *      that fails 2. is never converted and never cast.
 *   valid_out [N][M] uint8: 1 for a valid candidate, else 0 (whatever HK is).
 * Variant (e, m) is planned from env e's current state as heist_plan_masked plans one, HK =
 * min(horizon, max_steps - tick[e]) ticks (0 for an env already done), over
 *   vis_k(e, m) = base_vis[k-1][e] | cone_k(e, m),   k = 1 .. HK,
 * cone_k the tiles the candidate's rays mark on tick k: cast with the handle's ray_mode on the path
 * an env camera takes (fp32 fast path, tie buckets, exact recast of near-tie rays; exact-only above
 * range 6), the camera's own tile never marked by its own rays.  A camera of range 0 has no sample
 * and an empty cone (security.py:76-82), and so has an invalid candidate: such a variant is the
 * base rows' plan.
 *   ticks_out, value_out, action_out, togo_cells_out, value_cells_out: heist_plan_masked's outputs
 *            of the same names, shapes and alignments over those vis_k -- togo_0 and V_0 by
 *            heist_plan_field's and heist_plan_value's recurrences, V_0 in heist_plan_value's own
 *            arithmetic (the same lines in the same order, each one IEEE double operation, none
 *            contracted, the first maximum under a strict greater-than).
 *   vis_out  [horizon][N][M][W] uint32, 16-byte aligned, required (it is the backward sweeps'
 *            history): row (k-1, e, m), at (((k-1) N + e) M + m) W words, holds vis_k(e, m); the pad
 *            words are 0 and rows k > HK are 0, as in heist_plan_masked.
 * Every variant of an env with HK = 0 holds -1 / 0.0 / -1, in the cell tables too.
 * With heist_plan_field's rows as base_vis, a valid candidate's variant (range >= 1) is
 * heist_plan_field / heist_plan_value, bit for bit, on a handle built from the same layout with the
 * candidate appended to its camera list (budget + 3, one more camera slot) and brought to the same
 * state.
 * The launch only reads the env, as heist_plan_field does.
 * heist_plan_place_supported: heist_plan_masked_supported's value (the kernel's LDS is
 *   heist_plan_masked's): every grid up to 32 x 32 at 1, 2 and 4 K-tick waves; 64 x 64 is not
 *   supported.  -1 on a bad handle.
 * HEIST_EINVAL: horizon outside 1..1024, gamma not finite or outside [0, 1], M < 1 or N M >= 2^31,
 * a NULL cand, base_vis, valid_out, ticks_out, value_out, action_out or vis_out, base_vis or vis_out
 * not 16-byte aligned, cand, value_out or value_cells_out not 8-byte aligned, ticks_out or
 * togo_cells_out not 2-byte aligned, a probe mode armed (HEIST_PROBE_MODE),
 * heist_plan_place_supported 0. */
int heist_plan_place_supported(heist_t h);
int heist_plan_place(heist_t h, int horizon, double gamma, int M, const double* cand,
                     const uint32_t* base_vis, uint8_t* valid_out, int16_t* ticks_out, double* value_out,
                     int8_t* action_out, uint32_t* vis_out, int16_t* togo_cells_out,
                     double* value_cells_out, heist_stream_t stream);

/* Planner placement for guards, no reference counterpart: heist_plan_place's question with a guard
 * as the candidate -- M candidate guards per env in one launch, which tells where the Architect's
 * most expensive asset (5 points), and its only moving one, would have mattered.  The premise is the
 * camera's: an emitter blocks neither a ray nor a move, and a guard whose patrol starts on an EMPTY
 * tile leaves the wall plane alone (heist_set_layout marks only the start tile, as kGuard), so the
 * visibility of "this layout plus guard X" on a tick is the layout's own row OR X's cone OR X's own
 * cell on that tick.  The launch casts the candidate alone, against the env's wall plane; none of
 * the env's own emitters is read or cast.
 *   cand_path [N][M][P][2] int32, 4-byte aligned, 1 <= P <= 64: the patrol points (row, col) of
 *            candidate (e, m); only its first len points are read.
 *   cand_meta [N][M][4] int32, 4-byte aligned: len, speed, vision_range, idx.  idx is the patrol
 *            index the guard stands on now, at env e's current tick (0 for a guard as
 *            heist_set_layout leaves it).
 *   cand_fov  [N][M][2] float64, 8-byte aligned: fov_angle, heading.  heading is the guard's heading
 *            now (0.0 as heist_set_layout leaves it).
 *            The record is heist_set_layout's own conversion of an accepted guard: step = speed mod
 *            len (Python's %, never negative), range (int16)vision_range, max(int(fov_angle * 2),
 *            30) rays, pos0 = path[0], pos = path[idx], raycast live (no cone cache entry).  A
 *            heading with |heading| > 360, which no env guard ever holds (theirs is 0.0 or an entry
 *            of the handle's heading table), is first brought into [0, 360) by Python's % 360: the
 *            same direction.
 *   base_vis, gamma, horizon, M: heist_plan_place's, with the same meaning, layout and alignment.
 * Candidate (e, m) is valid iff all of these hold, every comparison false for a NaN:
 *   1. 1 <= len <= P and 0 <= idx < len;
 *   2. every one of the len points lies inside the grid, 0 <= r < R and 0 <= c < C
 *      (heist_set_layout's precondition; nothing is clamped here);
 *   3. path[0] is placeable as it stands (environment.py:160-167): 0 < r < R-1, 0 < c < C-1 and the
 *      tile is EMPTY.  Later points may be any tile, wall and border included: the env's guards
 *      walk such paths and the candidate does what they do;
 *   4. 0 < fov_angle <= 16000;
 *   5. |heading| <= 1e300;
 *   6. 0 <= vision_range < 32768.
 *   The budget, the guard slots and the handle's max_path are ignored: a handle created with
 *   max_guards = 0, or with no emitter slot at all, is served.  No int32 or float64 bit pattern in
 *   the three arrays makes the launch read or write out of bounds: the points are read only once
 *   1. and 4. - 6. hold, and an invalid candidate is never converted and never cast.
 *   valid_out [N][M] uint8: 1 for a valid candidate, else 0 (whatever HK is).
 * Variant (e, m) is planned as heist_plan_place plans one, HK = min(horizon, max_steps - tick[e])
 * ticks (0 for an env already done), over
 *   vis_k(e, m) = base_vis[k-1][e] | cone_k(e, m) | own cell_k(e, m),   k = 1 .. HK.
 * On tick k the guard first patrols (security.py:145-159): with len >= 2, idx = (idx + step) mod len
 * and pos = path[idx]; its heading becomes the handle's heading-table entry of the move when the
 * position changed, and is kept otherwise.  It then marks its own cell (visibility.py:59) and casts
 * from pos with the handle's ray_mode on the path a live-raycast env guard takes (whole-tile
 * samples; fp32 fast path, tie buckets, exact recast of near-tie rays; exact-only above range 6).
 * A range of 0 casts nothing and marks the own cell only.  An invalid candidate's variant is the
 * base rows' plan.
 *   ticks_out, value_out, action_out, vis_out, togo_cells_out, value_cells_out: heist_plan_place's
 *            outputs of the same names, shapes, alignments, padding and HK = 0 fill (-1 / 0.0 / -1,
 *            rows k > HK and pad words 0).
 * With heist_plan_field's rows as base_vis, a valid candidate's variant is heist_plan_field /
 * heist_plan_value, bit for bit, on a handle built from the same layout with the candidate appended
 * to its guard list (budget + 5, one more guard slot, max_path >= len) and brought to the same
 * state, whether that handle serves the guard from its cone cache or casts it live.  With the rows
 * of a heist_plan_masked variant that switches a guard off it is that guard's relocation.
 * The launch only reads the env.
 * heist_plan_place_guard_supported: heist_plan_place_supported's value.  -1 on a bad handle.
 * HEIST_EINVAL: horizon outside 1..1024, gamma not finite or outside [0, 1], M < 1 or N M >= 2^31,
 * P outside 1..64, a NULL cand_path, cand_meta, cand_fov, base_vis, valid_out, ticks_out, value_out,
 * action_out or vis_out, base_vis or vis_out not 16-byte aligned, cand_fov, value_out or
 * value_cells_out not 8-byte aligned, cand_path or cand_meta not 4-byte aligned, ticks_out or
 * togo_cells_out not 2-byte aligned, a probe mode armed (HEIST_PROBE_MODE),
 * heist_plan_place_guard_supported 0. */
int heist_plan_place_guard_supported(heist_t h);
int heist_plan_place_guard(heist_t h, int horizon, double gamma, int M, int P, const int32_t* cand_path,
                           const int32_t* cand_meta, const double* cand_fov, const uint32_t* base_vis,
                           uint8_t* valid_out, int16_t* ticks_out, double* value_out, int8_t* action_out,
                           uint32_t* vis_out, int16_t* togo_cells_out, double* value_cells_out,
                           heist_stream_t stream);

/* Planner walls, no reference counterpart: heist_plan_masked's two answers for every env with walls
 * added or removed -- M variants per env in one launch, which tells which wall a layout's difficulty
 * is due to, which wall the Solver hides behind, where one more wall would have mattered and whether
 * a wall keeps the level valid.  This is the case the three what-ifs above exclude: a wall stops
 * rays and moves, so a variant's visibility is no union over rows that already exist and its effect
 * is not monotone (a wall can help the Solver, and taking one away can hurt it).  Every variant is
 * therefore cast in full against its own edited stop map, and both recurrences run on its own
 * edited tile grid.
 *   edits        [N][M][E][3] int32, 4-byte aligned, 1 <= E <= 8: edit i of variant (e, m) is (row,
 *                col, op); op 0 is no edit (row and col are ignored), 1 adds a wall, 2 removes one.
 *   emitter_mask [N][M] uint64, 8-byte aligned, or NULL (every slot live): heist_plan_masked's mask
 *                with heist_plan_masked's meaning, so that "this camera off, a wall here" -- a camera
 *                moved behind a new wall, with heist_plan_place on top -- is one variant.
 * Every edit with op != 0 is judged against env e's grid as it stands, not as the variant's earlier
 * edits would leave it, and every comparison is decided before a byte is indexed:
 *   add (op 1):    valid iff 0 < r < R-1, 0 < c < C-1, tile (r, c) is EMPTY and it is not the Solver's
 *                  current cell (environment.py:160-167): not a wall, the start, the vault, a camera
 *                  or a guard's start tile.
 *   remove (op 2): valid iff 0 < r < R-1, 0 < c < C-1 and tile (r, c) is WALL.  The border stays; a
 *                  wall that a guard's start tile replaced is kGuard and cannot be removed.
 *   any other op:  invalid.
 * Variant (e, m) is valid iff every one of its edits with op != 0 is valid and no two of them name
 * the same tile.  No int32 pattern in edits makes the launch read or write out of bounds.
 *   valid_out [N][M] uint8: 1 for a valid variant, else 0 (whatever HK is).
 * An invalid variant is planned with no edit at all, under its mask: it is heist_plan_masked's
 * variant.  A valid variant is planned from env e's current state exactly as heist_plan_masked plans
 * one, HK = min(horizon, max_steps - tick[e]) ticks (0 for an env already done), on the edited tile
 * grid -- an added tile is WALL, a removed one EMPTY -- which is both the stop map the rays march
 * against and the grid the two backward sweeps read.  Every emitter record advances as in
 * heist_plan_masked.  Every live guard is raycast live in every variant, whether or not the handle
 * caches guard cones: a cone cached for the unedited walls is not the variant's.  A guard whose
 * patrol crosses an added wall walks onto it, marks its own cell there and casts from there, as an
 * env guard on a wall tile does.
 *   level_out [N][M] uint8: 1 iff the variant's grid (the unedited one for an invalid variant) still
 *             has a 4-neighbour path of non-WALL tiles from the handle's start tile -- not the
 *             Solver's cell -- to the vault: heist_bfs_valid's answer on that grid.  Where it is 0,
 *             HeistEnvironment.set_layout would have rejected the level; the variant is planned all
 *             the same (its ticks are -1 wherever the Solver is cut off).
 *   ticks_out, value_out, action_out, vis_out [horizon][N][M][W], togo_cells_out, value_cells_out:
 *             heist_plan_masked's outputs of the same names, shapes, alignments, padding and HK = 0
 *             fill (-1 / 0.0 / -1, rows k > HK and pad words 0), in heist_plan_masked's arithmetic
 *             (the same lines in the same order, each one IEEE double operation, none contracted,
 *             the first maximum under a strict greater-than).  In the cell tables an added wall cell
 *             holds -1 / 0.0 and a removed one a real value.
 * A variant with no edit of op != 0 is heist_plan_masked under the same mask, bit for bit, whether
 * or not the handle caches guard cones.  A valid variant with level_out 1 and every slot live is
 * heist_plan_field / heist_plan_value, bit for bit, on a handle built from the same layout with its
 * wall list edited -- the added tiles appended, the removed ones dropped, a budget that still buys
 * every asset -- and brought to the same state.
 * The launch only reads the env.
 * heist_plan_walls_supported: heist_plan_masked_supported's value (the kernel's LDS is
 *   heist_plan_masked's): every grid up to 32 x 32 at 1, 2 and 4 K-tick waves; 64 x 64 is not
 *   supported.  -1 on a bad handle.
 * HEIST_EINVAL: horizon outside 1..1024, gamma not finite or outside [0, 1], M < 1 or N M >= 2^31,
 * E outside 1..8, a NULL edits, valid_out, level_out, ticks_out, value_out, action_out or vis_out,
 * vis_out not 16-byte aligned, emitter_mask, value_out or value_cells_out not 8-byte aligned, edits
 * not 4-byte aligned, ticks_out or togo_cells_out not 2-byte aligned, a probe mode armed
 * (HEIST_PROBE_MODE), heist_plan_walls_supported 0. */
int heist_plan_walls_supported(heist_t h);
int heist_plan_walls(heist_t h, int horizon, double gamma, int M, int E, const int32_t* edits,
                     const uint64_t* emitter_mask, uint8_t* valid_out, uint8_t* level_out,
                     int16_t* ticks_out, double* value_out, int8_t* action_out, uint32_t* vis_out,
                     int16_t* togo_cells_out, double* value_cells_out, heist_stream_t stream);

/* Planner playout, no reference counterpart: one episode per env played from a planner's per-tick
 * tables -- the table's own (expert) play, or that play perturbed on a counter-hashed share of the
 * steps, every visited state still labelled by the table.  The emitters do not depend on the
 * Solver, so the play is a function of the visibility rows, the grid, the start cell and the
 * action rule: no ray is cast and no env is touched.  Env e plays HK = min(horizon, max_steps -
 * tick[e]) steps, 0 for an env already done; x_0 is pos0[e], or the env's cell when pos0 is NULL.
 * With move(x, a) as in heist_plan_field, for k = 0 .. HK-1 while the play is live:
 *   t = action_table[k][e][x_k], the expert's action; an entry outside 0 .. 4 is stored as -1 in
 *       expert_out and played as WAIT;              value_out[k][e] = value_table[k][e][x_k]
 *   z = mix64(seed ^ (tick[e] + k) * 0xD1B54A32D192ED03 ^ e * 0x9E3779B97F4A7C15)   (mod 2^64),
 *       mix64 as under heist_solver_head; the step is noisy iff (z >> 40) < noise_q24 (0: never,
 *       2^24: always) and then takes a = ((z & 0xFFFFFFFF) * 5) >> 32, else a = t (WAIT for an
 *       invalid t).  The key holds the env's absolute tick: a call made mid-episode with the same
 *       seed continues with the same draws.
 *   y = move(x_k, a);  seen = bit y of vis[k][e];  x_{k+1} = y
 *   the step's reward is heist_plan_value's rew with x = x_k, line for line, each line one IEEE
 *       double operation, none contracted, last = tick[e] + k + 1 >= max_steps; it equals the env's
 *       reward64 of the same actions whenever prev_dist = dist(x_0)
 *   status = HEIST_RUNNING, then HEIST_DETECTED if seen, then HEIST_VAULT_REACHED if y is the
 *       vault, then HEIST_TIMEOUT if last (the env's own precedence); done = any of the three
 *   records_out[k][e] is the compact record of the observation after the step: the visibility
 *       words are vis[k][e]'s, the position word is y_r | y_c << 8, the padding words are 0
 * The play ends after a done step; len_out[e] is the number of steps played.  Rows after the end,
 * and every row of an env with HK = 0, hold action 0, expert -1, value 0.0, a zero record, reward
 * 0.0, done 1 and status HEIST_ALREADY_DONE; a play the horizon cuts has no such rows.
 *   action_table [horizon][N][R*C] int8, required: e.g. heist_plan_value's action_ticks_out
 *   vis          [horizon][N][W] uint32, 16-byte aligned, required: heist_plan_field's /
 *                heist_plan_value's vis_out of the same handle state
 *   value_table  [horizon][N][R*C] float64 or NULL, 8-byte aligned: value_ticks_out
 *   pos0         [N][2] int32 (r, c) or NULL.  A cell outside the grid is found on the device:
 *                that env plays nothing, all its rows hold the fill and len_out[e] is -1
 *   actions_out  [horizon][N] int64, required: heist_step_multi's `actions` as it stands
 *   expert_out   [horizon][N] int8 or NULL;  value_out [horizon][N] float64 or NULL (needs
 *                value_table);  records_out [horizon][N][W] uint32 or NULL, 16-byte aligned;
 *                reward64_out [horizon][N] float64 or NULL
 *   done_out     [horizon][N] uint8 and status_out [horizon][N] int8, required
 *   len_out      [N] int32 or NULL
 * The launch only reads the handle (the envs' scalars and grids), as the planners do; every grid
 * up to 64 x 64 is served (a hand-made table plays where heist_plan_value has no kernel).
 * HEIST_EINVAL: horizon outside 1..1024, a NULL action_table, vis, actions_out, done_out or
 * status_out, value_out without value_table, vis or records_out not 16-byte aligned, value_table,
 * value_out, reward64_out or actions_out not 8-byte aligned, noise_q24 > 2^24. */
int heist_plan_play(heist_t h, int horizon, const int8_t* action_table, const uint32_t* vis,
                    const double* value_table, const int32_t* pos0, uint32_t noise_q24, uint64_t seed,
                    int64_t* actions_out, int8_t* expert_out, double* value_out, uint32_t* records_out,
                    double* reward64_out, uint8_t* done_out, int8_t* status_out, int32_t* len_out,
                    heist_stream_t stream);

/* Planner Q, no reference counterpart: the five exact action values of every visited state -- the
 * one-step lookahead heist_plan_value's recurrence defines, on caller-chosen states instead of
 * every cell -- with their maximum, the set of optimal actions and the loss of the action taken.
 * t0[e] is tick0[e], or with tick0 NULL the env's tick now (-1 for an env that is done now): the
 * env's tick when the tables were made, -1 for an env that was done then, which lets a rollout be
 * labelled after the handle has been stepped through it.  Env e has HK = min(horizon, max_steps -
 * t0[e]) steps, 0 for t0[e] < 0.  A state is (k, e, x = pos[k][e]), the cell the Solver stands on
 * k ticks after t0 (row 0 the cell then: heist_amd.search.expert_labels' convention); it is live
 * when k < HK, x is inside the grid and x is not a wall cell.  For a live state and a = 0 .. 4 in
 * order, with y = move(x, a) as in heist_plan_field,
 *   q[a] = heist_plan_value's q of (x, a, k), line for line, each line one IEEE double operation,
 *          none contracted: rew (its six lines), seen = bit y of vis[k][e], last = t0[e] + k + 1 >=
 *          max_steps, q = (seen or y == vault or last) ? rew : rew + gamma * V_{k+1}[y], where
 *          V_{k+1}[y] is value_table[k+1][e][y] when k + 1 < horizon, else 0.0
 *   value = the maximum q under a strict greater-than, best = its first a: for tables made by
 *          heist_plan_value with the same gamma on the same handle state they equal
 *          value_ticks_out[k][e][x] and action_ticks_out[k][e][x] bit for bit
 *   optimal: bit a is set iff q[a] == value (exact double equality; a blocked move that ties with
 *          an optimal WAIT is in the set: it is the same transition)
 *   gap = value - q[taken[k][e]], one subtraction; an entry of taken outside 0 .. 4 counts as WAIT,
 *          as in heist_plan_play.  gap is exactly 0.0 iff the taken action is in the optimal set.
 * A state that is not live holds q = 0.0 five times, value 0.0, best -1, optimal 0 and gap 0.0.
 *   value_table [horizon][N][R*C] float64, 8-byte aligned, required: e.g. value_ticks_out
 *   vis         [horizon][N][W] uint32, 16-byte aligned, required: heist_plan_value's /
 *               heist_plan_field's vis_out (row k holds vis_{k+1})
 *   tick0       [N] int32 or NULL;  pos [K][N][2] int32 (r, c), 1 <= K <= horizon, required
 *   taken       [K][N] int64 or NULL
 *   q_out [K][N][5] float64, value_out [K][N] float64, best_out [K][N] int8, optimal_out [K][N]
 *               uint8, gap_out [K][N] float64 (needs taken): each may be NULL, not all of them
 * From the handle the launch reads only what does not change within an episode -- the grid, the
 * vault, initial_dist, max_steps and reward_consts (and, with tick0 NULL, tick and done) -- so the
 * handle's layout must be the one the tables were made for; it writes the caller's arrays alone.
 * Every grid up to 64 x 64 is served (no LDS array per cell: a hand-made table is labelled where
 * heist_plan_value has no kernel).
 * HEIST_EINVAL: horizon outside 1..1024, K outside 1..horizon, gamma not finite or outside [0, 1],
 * a NULL value_table, vis or pos, every output NULL, gap_out without taken, vis not 16-byte
 * aligned, value_table, taken, q_out, value_out or gap_out not 8-byte aligned, tick0 or pos not
 * 4-byte aligned, a probe mode armed (HEIST_PROBE_MODE). */
int heist_plan_q(heist_t h, int horizon, int K, double gamma, const double* value_table, const uint32_t* vis,
                 const int32_t* tick0, const int32_t* pos, const int64_t* taken, double* q_out, double* value_out,
                 int8_t* best_out, uint8_t* optimal_out, double* gap_out, heist_stream_t stream);

/* Instrumentation, no reference counterpart: with counter a device array of n_envs uint64,
 * every later heist_step / heist_reset on h adds to counter[e] the number of ray samples
 * env e evaluated (the ALU work figure of SURVEY 8(d)); NULL switches counting off (default). */
int heist_count_samples(heist_t h, uint64_t* counter);

/* Instrumentation, no reference counterpart: like heist_count_samples, counter[e] += the
 * number of env e's rays whose fp32 fast path met a near .5 tie and were re-cast on the
 * exact fp64 path. */
int heist_count_redo(heist_t h, uint64_t* counter);

/* Instrumentation, no reference counterpart: later heist_step calls on h record the shader
 * clock (s_memtime) at 8 phase boundaries of every wavefront into buf[env][wave][10] (waves
 * per env: heist_step_waves(h); slots 8 and 9 hold HW_ID and XCC_ID): 0 entry, 1 prefetch
 * landed, 2 emitter table published, 3 raycast done, 4 reward done, 5 auto-reset done, 6
 * observation written, 7 exit.  heist_step_multi writes buf[env][multi_waves][16] instead:
 * clock cycles summed per tick segment 0..8 over the launch, lifetime, start clock, HW_ID,
 * XCC_ID.  n_words is buf's size in uint64 words: a call whose kernel needs more
 * (n_envs * 10 * step_waves, resp. n_envs * 16 * multi_waves; heist_stamp_words reports both)
 * fails with HEIST_EINVAL instead of writing past it.  NULL switches stamping off (default). */
int heist_step_stamps(heist_t h, uint64_t* buf, int64_t n_words);

/* uint64 words of a stamp buffer for heist_step (which = 0) or heist_step_multi (which = 1)
 * on h; no reference counterpart. */
int64_t heist_stamp_words(heist_t h, int which);

/* Wavefronts per env of h's step / reset kernels (2 unless HEIST_STEP_WAVES chose 1 or 4
 * at heist_create); no reference counterpart. */
int heist_step_waves(heist_t h);

/* The handle's effective kernel configuration, no reference counterpart (what a benchmark
 * records next to its numbers): out[0..n) with n <= 16 receives step_waves, ray_chunk,
 * step_occ, vis_gap, obs_store, ray_mode, probe_mode, dispatch_order, split_obs,
 * guard_cones, multi_waves, fan_on, lean, interval_fans (the HEIST_* environment knobs as heist_create resolved them,
 * then any heist_set_* calls), step_lean (1: heist_step currently runs as a one-tick
 * heist_step_multi launch on the lean kernel; HEIST_STEP_LEAN=1 at heist_create turns it on),
 * lean_waves (waves per env of the lean kernel as a heist_step_multi launch would run it now:
 * 2 for the 32 x 32 kernel when the batch's doubled waves fit the chip, HEIST_LEAN_WAVES=1/2
 * forces; 1 with stamps armed, and 1 when the lean kernel does not serve the handle).
 * ray_chunk, step_occ and dispatch_order always report 4, 8 and 1: their knobs (samples per
 * ray chunk, waves per SIMD the step kernel is built for, block -> env order: heaviest raycast
 * first) were measured, removed (profiles/r01m_*, r02bd_probe_dispatch_order.log,
 * r05e_configs_*), and the words keep their places for the ABI.  probe_mode != 0 selects the profiling step kernel, whose results are
 * wrong by design (phases skipped). */
int heist_get_config(heist_t h, int32_t* out, int n);

/* Raycast arithmetic of later heist_step / heist_reset calls on h: 0 (default) = fp32 fast
 * path with exact fp64 re-cast of every ray that comes within a bounded error of a .5 tie,
 * 1 = exact fp64 path for every ray.  Both give bit-identical visibility; 1 exists for
 * parity tests and A/B timing.  The environment variable HEIST_EXACT_RAYS=1 sets 1 at
 * heist_create. */
int heist_set_ray_mode(heist_t h, int ray_mode);

/* Guard cone cache, no reference counterpart (a precomputation of Guard.get_visible_tiles,
 * security.py:161-192): with on = 1 (default; HEIST_GUARD_CONES=0 at heist_create turns
 * it off) every later heist_set_layout casts each guard's vision cone once per (patrol
 * index, heading) on the exact fp64 path, and heist_step / heist_reset OR the cached cone
 * instead of raycasting the guard (guards with a patrol of more than 16 points, more than
 * 8 distinct headings or a vision range above 7 are always raycast).  Results are
 * identical either way; on = 0 raycasts every guard every tick.  Takes effect at the next
 * heist_set_layout. */
int heist_set_guard_cones(heist_t h, int on);

/* Replaces bfs_path_exists (utils.py:52-85) on a batch of grids [N][R][C] int32. */
int heist_bfs_valid(const int32_t* grid, int n, int rows, int cols, int start_r, int start_c, int goal_r,
                    int goal_c, uint8_t* valid_out, heist_stream_t stream);

/* Replaces Camera.get_vision_cone_tiles (security.py:53-101, kind 0) and
 * Guard.get_visible_tiles (security.py:161-192, kind 1) for n independent emitters:
 *   walls [n][R][C] uint8 (nonzero = wall); meta [n][4] int32 = kind, row, col, range;
 *   params [n][2] f64 = fov_angle, heading;  tiles_out [n][R][C] uint8 (1 = visible). */
int heist_cones(int n, int rows, int cols, const uint8_t* walls, const int32_t* meta, const double* params,
                uint8_t* tiles_out, heist_stream_t stream);

/* The reference's LIST ORDER of the same cones (get_vision_cone_tiles / get_visible_tiles
 * append a tile when a ray first reaches it, rays in index order, samples in distance
 * order): keys_out [n][R][C] uint32 = (ray << 12 | sample) of the first visit on the exact
 * fp64 path, 0xFFFFFFFF where no ray reaches the tile.  Same inputs as heist_cones. */
int heist_cone_order(int n, int rows, int cols, const uint8_t* walls, const int32_t* meta, const double* params,
                     uint32_t* keys_out, heist_stream_t stream);

/* heist_cones with an explicit ray_mode (0 fast + exact re-cast, 1 exact only; see
 * heist_set_ray_mode).  heist_cones is ray_mode 0. */
int heist_cones_mode(int n, int rows, int cols, const uint8_t* walls, const int32_t* meta, const double* params,
                     int ray_mode, uint8_t* tiles_out, heist_stream_t stream);

/* The fast path's fp32 ray direction for angles in degrees (parity tooling: its error
 * against the exact glibc direction bounds the near-tie tolerance).  [n] f64 in,
 * cos_out, sin_out [n] f32. */
int heist_fast_dir(const double* angle_deg, int64_t n, float* cos_out, float* sin_out, heist_stream_t stream);

/* Replaces the decode half of ArchitectNetwork.generate_layout (networks.py:283-335) and
 * the curriculum filter of training.py:464-467 for n sampled layouts:
 *   asset_map [n][R][C] int64 per-cell class (0 none, 1 wall, 2 camera, 3 guard);
 *   cam_params [3] or [n][3] float32 = fov, speed, heading (cam_stride 0 or 3);
 *   budget [n] int32.  Outputs are the heist_set_layout input arrays with capacities
 *   max_walls / max_cams / max_guards / max_path (max_path >= 8); lists longer than a
 *   capacity are truncated, so size capacities from the budget (budget, /3, /5).  Only the
 *   first n_walls / n_cams / n_guards entries of an env are written; with allow_cams or
 *   allow_guards 0 that list's count is 0 (its assets still cost their budget in the scan). */
int heist_architect_decode(const int64_t* asset_map, int n, int rows, int cols, const float* cam_params,
                           int cam_stride, const int32_t* budget, int allow_cams, int allow_guards, int max_walls,
                           int max_cams, int max_guards, int max_path, int32_t* wall_rc, int32_t* n_walls,
                           double* cam_out, int32_t* n_cams, int32_t* guard_paths, int32_t* guard_meta,
                           double* guard_fov, int32_t* n_guards, heist_stream_t stream);

/* math.sin / math.cos of the reference's raycast (security.py:74-75, :174-175) as the GPU
 * evaluates them: glibc 2.35's dbl-64 algorithm, bit-exact to the host libm for
 * |x| < 105414350.  x, sin_out, cos_out [n] float64 (parity checks and tooling). */
int heist_sincos(const double* x, int64_t n, double* sin_out, double* cos_out, heist_stream_t stream);

/* Replaces the Architect's per-layout update cadence (training.py:479-480 / :558-559:
 * ArchitectAgent.update after every layout with ONE transition, agents/architect.py:91-155)
 * for k consecutive rewards, as one persistent launch (64 workgroups, one per CU, grid
 * barriers between phases).  With one transition update i is an Adam step on
 * value_coeff * (V(s0) - rewards[i])^2, V = ArchitectNetwork's value path (encoder ->
 * adaptive pool -> fc_global -> value_head, networks.py:159-188) on the constant grid s0,
 * after clip_grad_norm_(max_norm) over the 12 value-path tensors.  Workgroup w owns conv2 /
 * conv3 channels 4(w%16)..+3 on pool-cell row band w/16 of the image.
 *   params / exp_avg / exp_avg_sq: HOST arrays of 12 device pointers each, in
 *     ArchitectNetwork.parameters() order restricted to the value path: encoder.0.weight
 *     [32][1][3][3], encoder.0.bias, encoder.2.weight [64][32][3][3], encoder.2.bias,
 *     encoder.4.weight [64][64][3][3], encoder.4.bias, fc_global.weight [256][1024],
 *     fc_global.bias, value_head.0.weight [128][256], value_head.0.bias,
 *     value_head.2.weight [1][128], value_head.2.bias; float32, contiguous; the weights of
 *     encoder.2 / encoder.4 / value_head.0 128-byte aligned.  Updated in place.
 *   grid [rows][cols] float32 = s0 with at most 64 nonzero pixels (the Architect's state
 *     has 2);  rewards [k] float32;  value_loss [k] float32 out
 *     (mse of each step, before its update).
 *   step_scalars [k][2] float32 (device): per update, the two scalars torch.optim.Adam forms
 *     in float64 from the step count and casts to float: -lr / (1 - beta1^step) and
 *     sqrt(1 - beta2^step); beta1, beta2, eps as torch.optim.Adam (amsgrad, weight_decay,
 *     maximize off; the foreach arithmetic).
 *   workspace: heist_arch_update_workspace_bytes() device bytes, not shared by launches in
 *     flight.  rows x cols in {8, 12, 16, 20} squared (heist_arch_update_supported). */
int64_t heist_arch_update_workspace_bytes(void);
int heist_arch_update_supported(int rows, int cols);
int heist_arch_update_sequence(float* const* params, float* const* exp_avg, float* const* exp_avg_sq,
                               const float* grid, int rows, int cols, const float* rewards, int k,
                               const float* step_scalars, double beta1, double beta2, double eps, double max_norm,
                               double value_coeff, float* value_loss, void* workspace, heist_stream_t stream);
/* Status of the last launch on `workspace`, a bit mask; any bit set means its results --
 * the updated params, exp_avg, exp_avg_sq and value_loss -- are INVALID (the caller restores
 * its own copy and re-runs the steps another way):
 *   bit 0: a grid barrier gave up waiting (the 64 workgroups were not co-resident; the spin
 *          bound is 2^25 polls, HEIST_ARCH_SPIN_LIMIT overrides it, e.g. to test this path);
 *   bit 1: grid has more than 64 nonzero pixels.
 * The word is the uint32 at byte offset heist_arch_update_workspace_bytes() - 252 of the
 * workspace (zeroed at each launch), so a caller can also copy it asynchronously.
 * Synchronises `stream`.  heist_arch_update_timed_out reports bit 0 alone. */
int heist_arch_update_status(const void* workspace, int* status, heist_stream_t stream);
int heist_arch_update_timed_out(const void* workspace, int* timed_out, heist_stream_t stream);
/* Instrumentation, no reference counterpart: with buf a device array of 2 * 16 * 32 + 16 * 5 * 64
 * uint64, later heist_arch_update_sequence launches record s_memrealtime (100 MHz) at up to 32
 * phase points of steps 0..15 in workgroups 0 and 63, then every workgroup's arrival (stores
 * drained) at each of the 5 grid barriers of steps 0..15 (tools/probe_arch_update.py); NULL: off. */
int heist_arch_update_stamps(uint64_t* buf);

/* The batched trainer's per-tick attempt bookkeeping over n envs (the per-episode counters of
 * training.py:515-544 -- steps, reward, outcome per attempt -- and solver.reset() per attempt,
 * :517), replacing ~20 tensor ops per tick: counting = valid[e] && attempts[e] <
 * attempts_per_layout; steps += counting; reward_sum += counting ? reward64 : 0.0 (float64);
 * an attempt that ends (counting && done) adds 1 to solve (status 2 = vault_reached), detect
 * (status 1) or timeout (any other status) and to attempts; h, c [n][hidden] float32 (the
 * LSTM state, layer dimension 1) are multiplied by (done ? 0 : 1).  valid, done uint8 (bool),
 * status int8, the counters int32. */
/* The Solver's LSTM cell after its gate GEMMs (reference networks.py:90-100, nn.LSTM one time
 * step, gate order i, f, g, o; replaces the ten pointwise torch kernels of
 * SolverNetwork.lstm_step in the rollout): gates = gates_x + gates_h ([n][4 hidden] float32
 * each), c_out = sigmoid(f) * c + sigmoid(i) * tanh(g), h_out = sigmoid(o) * tanh(c_out)
 * ([n][hidden]), every operation rounded to float32 in that order (bit-identical to torch's
 * kernels). */
int heist_lstm_cell(const float* gates_x, const float* gates_h, const float* c, float* h_out, float* c_out, int hidden,
                    int n, heist_stream_t stream);

int heist_rollout_tally(const uint8_t* valid, int32_t* attempts, int attempts_per_layout, const uint8_t* done,
                        const int8_t* status, const double* reward64, int32_t* steps, double* reward_sum, int32_t* solve,
                        int32_t* detect, int32_t* timeout, float* h, float* c, int hidden, int n, heist_stream_t stream);

/* Replaces SolverAgent._compute_gae + returns (agents/solver.py:142-143, :228-244) on a
 * [T][N] rollout (column e = env e's concatenated episodes).  dones [T][N] uint8.
 * last_value [N] bootstraps t = T-1 (NULL = 0, the reference's buffer-end rule).  gamma and
 * lam are taken in float64 because the reference forms gamma*lam in Python floats. */
int heist_gae(const float* rewards, const float* values, const uint8_t* dones, const float* last_value,
              int T, int n, double gamma, double lam, float* adv_out, float* ret_out, heist_stream_t stream);

/* Advantage normalisation (agents/solver.py:146-147): x <- (x - mean) / (std + eps),
 * unbiased std; skipped when the global count is <= 1.  acc is a device float64[3] the
 * caller zeroes.  Phases (multi-GPU callers all-reduce acc between them):
 *   phase 0: acc[0] += sum(x), acc[1] += n            -> all-reduce acc[0..1]
 *   phase 1: acc[2] += sum((x - acc[0]/acc[1])^2)     -> all-reduce acc[2]
 *   heist_adv_apply(x, n, acc, eps)
 * heist_adv_normalize runs both phases and the apply on one device (acc = scratch3). */
int heist_adv_moments(const float* x, int64_t n, int phase, double* acc, heist_stream_t stream);
int heist_adv_apply(float* x, int64_t n, const double* acc, float eps, heist_stream_t stream);
int heist_adv_normalize(float* x, int64_t n, double* scratch3, float eps, heist_stream_t stream);

/* Clipped PPO loss of SolverAgent.update (agents/solver.py:172-193) over M samples with
 * Categorical(probs=softmax(logits)) semantics, fused forward + backward:
 *   logits [M][A] f32 (A <= 16), values [M] f32, actions [M] int64, old_logp/adv/ret [M] f32;
 *   loss_parts [4] f32 = total, policy, value, entropy (means over M);
 *   dlogits [M][A], dvalues [M] = d(total)/d(input);  scratch >= 3*ceil(M/256) float64. */
int heist_ppo_loss(const float* logits, const float* values, const int64_t* actions, const float* old_logp,
                   const float* adv, const float* ret, int M, int A, double clip, double vcoef, double ecoef,
                   float* loss_parts, float* dlogits, float* dvalues, double* scratch, heist_stream_t stream);

/* Fused batched SolverNetwork backbone (networks.py:93-100: relu(conv1) -> relu(conv2) ->
 * relu(conv3) -> AdaptiveAvgPool2d(4,4) -> flatten) on bf16 MFMA with fp32 accumulation,
 * for SolverAgent.select_action (agents/solver.py:75-99) over a batch.
 * heist_solver_pack converts the float32 torch parameters conv{1,2,3}.weight [co][ci][3][3]
 * and .bias [co] (3->32->64->64) into the kernel's fragment layout in `packed`
 * (heist_solver_packed_bytes() bytes, 16-byte aligned); call it after every weight update.
 * heist_solver_features: obs [n][3][rows][cols] float32 -> feat_out [n][1024] float32
 * (channel-major 64 x 4 x 4, the x.view(batch, -1) order).  rows x cols in {20x20, 10x10, 32x32};
 * other sizes return HEIST_EINVAL (callers use the PyTorch path). */
int heist_solver_packed_bytes(void);
int heist_solver_pack(const float* conv1_w, const float* conv1_b, const float* conv2_w, const float* conv2_b,
                      const float* conv3_w, const float* conv3_b, void* packed, heist_stream_t stream);
int heist_solver_features(const float* obs, int n, int rows, int cols, const void* packed, float* feat_out,
                          heist_stream_t stream);

/* Fused batched Solver head (networks.py:102-131 + agents/solver.py:75-99 select_action):
 * x = relu(fc_spatial(feat)); one LSTM cell step (gate order i, f, g, o); logits =
 * policy_head(h'), value = value_head(h'); action ~ Categorical(softmax(logits)) and its
 * log_prob with torch's probs semantics.  GEMMs on bf16 MFMA (fp32 accumulate), cell
 * update, last layers and sampling in fp32.  Requires hidden_dim 256, lstm_hidden 128,
 * head width 128, 1 <= num_actions <= 7.
 * heist_solver_head_pack: float32 parameters (torch layouts: fc_spatial.weight [256][1024],
 * lstm.weight_ih_l0 [512][256], weight_hh_l0 [512][128], policy_head.0 / value_head.0
 * .weight [128][128], policy_head.2.weight [A][128], value_head.2.weight [1][128], biases)
 * -> packed (heist_solver_head_packed_bytes() bytes); call after every weight update.
 * heist_solver_head: feat [n][1024] (heist_solver_features), h_in / c_in [n][128] or NULL
 * (zero state); seed / counter select the sample (counter-based hash, one uniform per env);
 * outputs logits [n][A] (may be NULL), value [n], action [n] int64, logp [n],
 * h_out / c_out [n][128] (must not alias h_in / c_in).  h_in and c_in are independently
 * optional; rows past n - 1 of no output are written; n == 0 is a no-op.
 * The draw is part of the contract (saved runs replay it): for env e of the batch,
 *   z = mix64(seed ^ counter * 0xD1B54A32D192ED03 ^ e * 0x9E3779B97F4A7C15)   (mod 2^64),
 *   mix64(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 *             z ^= z >> 31                                     (the splitmix64 finaliser),
 *   u = (z >> 40) * 2^-24                                      (the top 24 bits, 0 <= u < 1),
 * with p = softmax(logits) in fp32 and S = p_0 + ... + p_{A-1},
 *   action = the first a with u * S < p_0 + ... + p_a, else A - 1
 * (strict: a draw on a boundary takes the action above it, and an action of probability 0
 * is never taken), and logp = log(clamp(p_action / S, eps, 1 - eps)) with eps = 2^-23
 * (fp32 epsilon), which is torch's Categorical(probs=p).log_prob(action). */
/* Instrumentation, no reference counterpart: with buf a device array of
 * n_workgroups * 4 * 10 uint64, later heist_solver_features launches record s_memtime at
 * 10 phase points of each wave for its workgroup's second env (tools/probe_policy.py);
 * NULL switches it off (default). */
int heist_solver_stamps(uint64_t* buf);

int heist_solver_head_packed_bytes(void);
int heist_solver_head_pack(const float* fc_w, const float* fc_b, const float* w_ih, const float* w_hh,
                           const float* b_ih, const float* b_hh, const float* p1_w, const float* p1_b,
                           const float* v1_w, const float* v1_b, const float* p2_w, const float* p2_b,
                           const float* v2_w, const float* v2_b, int num_actions, void* packed,
                           heist_stream_t stream);
int heist_solver_head(const float* feat, const float* h_in, const float* c_in, int n, const void* packed,
                      int num_actions, uint64_t seed, uint64_t counter, float* logits_out, float* value_out,
                      int64_t* action_out, float* logp_out, float* h_out, float* c_out, heist_stream_t stream);

/* The Solver backbone's fp32 training step (agents/solver.py:157-199 over networks.py:93-100:
 * relu(conv1) -> relu(conv2) -> relu(conv3) -> AdaptiveAvgPool2d(4, 4), forward and backward)
 * with the convolutions run without bias (MIOpen) and everything between them fused into one
 * pass per layer.  Tensors are NHWC (channels_last) fp32, 16-byte aligned; n samples of rows x
 * cols positions.
 *   heist_bias_relu_nhwc: x[p][c] = relu(x[p][c] + bias[c]) in place (F.relu(conv + b)).
 *   heist_bias_relu_pool_nhwc: the same for conv3 (64 channels) plus feat_out [n][64 * 16] =
 *     adaptive_avg_pool2d(., (4, 4)) flattened C-major (the view fc_spatial reads).
 *   heist_pool_relu_bwd_nhwc: the backward of the two: d_out = (y > 0) * (the pool's input
 *     gradient of dfeat [n][1024]) (conv3's grad_output), dbias_out [64] = its sum over
 *     samples and positions; partial: [n][64] floats of scratch.
 *   heist_relu_bwd_nhwc: g = (y > 0) ? g : 0 in place (threshold_backward on the saved output)
 *     and dbias_out [channels] its sum; partial [n][channels] scratch; 32 or 64 channels.
 * Sums run in a fixed order (deterministic; fp32 rounding differs from torch's order). */
int heist_bias_relu_nhwc(float* x, const float* bias, int64_t n_pos, int channels, heist_stream_t stream);
int heist_bias_relu_pool_nhwc(float* x, const float* bias, int n, int rows, int cols, int channels, float* feat_out,
                              heist_stream_t stream);
int heist_pool_relu_bwd_nhwc(const float* dfeat, const float* y, int n, int rows, int cols, int channels, float* d_out,
                             float* partial, float* dbias_out, heist_stream_t stream);
int heist_relu_bwd_nhwc(float* g, const float* y, int n, int positions, int channels, float* partial, float* dbias_out,
                        heist_stream_t stream);

/* The Solver backbone's fp32 training convolutions on fp32 MFMA (v_mfma_f32_16x16x4_f32, exact
 * fp32), for the PPO update's forward and backward (agents/solver.py:157-199 over
 * networks.py:93-100): every pass of relu(conv1) -> relu(conv2) -> relu(conv3) -> pool as one
 * persistent kernel with the weights in registers and the activation bands in LDS, replacing
 * MIOpen's convolutions.  20 x 20 and 32 x 32 grids (heist_train_conv_supported: bands of 4
 * and of 2 image rows per work unit; any other size is rejected).  Activations are
 * [n][rows][cols][P] float32 with P = channels + 4 (the 4 pad words are never read), the
 * network input [n][rows][cols][4] (heist_train_obs_nhwc4), all 16-byte aligned.
 *   heist_train_conv_pack: torch weights [co][ci][3][3] of layer 1 (3 -> 32, mode 0), 2 (32 -> 64)
 *     or 3 (64 -> 64) -> frag (heist_train_conv_frag_floats floats); mode 0 the forward
 *     convolution, mode 1 its data gradient (transposed, flipped taps).
 *   heist_train_conv: mode 0 y = relu(conv(x) + bias) and, if mask_bits is not NULL, its ReLU
 *     mask as bits (ReLU masks are [n][rows][cols][channels / 4] uint8: bit r of byte k =
 *     channel 4 k + r is > 0); mode 1 (layers 2, 3) y = mask ? conv_data_grad(x) : 0 with x the
 *     gradient at the layer's output (64 channels) and mask_bits the mask of the layer's input
 *     (the forward's bits of the layer below: threshold_backward).  queue: 2 device ints, zero
 *     before the first launch (the kernels leave them zero); one pair per launch in flight.
 *   heist_train_conv_wgrad: dw [co][ci][3][3] and db [co] of layer 1-3 from dy (the gradient at
 *     the layer's pre-activation output) and x (its input); partial:
 *     heist_train_conv_partial_floats(layer, n, ...) floats of scratch.  Sums in a fixed order.
 *   heist_train_obs_nhwc4: obs [n][3][rows][cols] with element strides -> [n][rows][cols][4].
 *   heist_train_pool: feat [n][1024] = adaptive_avg_pool2d(a3, (4, 4)) flattened C-major.
 *   heist_train_pool_bwd: d3 = mask3 * the pool's input gradient of dfeat [n][1024], mask3 the
 *     ReLU mask bits of conv3's forward. */
int heist_train_conv_supported(int rows, int cols);
int heist_train_conv_frag_floats(int layer, int mode);
int heist_train_conv_pack(int layer, int mode, const float* w, float* frag, heist_stream_t stream);
int heist_train_conv(int layer, int mode, const float* x, int n, int rows, int cols, const float* frag,
                     const float* bias, uint8_t* mask_bits, float* y, int* queue, heist_stream_t stream);
int64_t heist_train_conv_partial_floats(int layer, int n, int rows, int cols);
int heist_train_conv_wgrad(int layer, const float* dy, const float* x, int n, int rows, int cols, float* partial,
                           float* dw, float* db, int* queue, heist_stream_t stream);
int heist_train_obs_nhwc4(const float* obs, int n, int rows, int cols, int64_t stride_n, int64_t stride_c,
                          int64_t stride_h, int64_t stride_w, float* x4, heist_stream_t stream);
int heist_train_pool(const float* a3, int n, int rows, int cols, float* feat, heist_stream_t stream);
int heist_train_pool_bwd(const float* dfeat, const uint8_t* mask3_bits, int n, int rows, int cols, float* d3,
                         heist_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
