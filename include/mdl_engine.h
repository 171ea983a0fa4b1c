/*
 * mdl_engine.h -- C ABI of the MI355X-native marl-delivery batched step engine.
 *
 * One engine = E independent grid-world instances resident in HBM on one GPU.
 * All compute runs as gfx950 HIP kernels, one wavefront per env instance.
 * Entry points are extern "C", take plain pointers and sizes, and return an
 * int status (0 = ok, <0 = error; mdl_last_error() gives a thread-local
 * message).  No exception crosses the ABI.  Every call that takes a `stream`
 * (a hipStream_t passed as void*, NULL = default stream) is asynchronous on
 * that stream; device pointers are caller-owned unless documented otherwise.
 * One engine per device; calls on one handle are not thread-safe.
 *
 * The reference has no FFI (it is pure Python); each entry point below names
 * the Python interface it replaces (path:line under the reference tree).
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference
 * would add.
 */
#ifndef MDL_ENGINE_H
#define MDL_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDL_MAX_ROBOTS 64      /* one wavefront lane per robot */
#define MDL_MAX_PACKAGES 1024  /* Group-Project.pdf p.3 bounds G <= 1000 */
#define MDL_MAX_CELLS 16384    /* H*W <= 128*128; H, W <= 255 */

/* tracker semantics of the persistent-package dict */
#define MDL_TRACKER_FRESH 0        /* == env truth; QMIX/trainer.py:523-526 clears it on reset */
#define MDL_TRACKER_MAPPO_STALE 1  /* MAPPO/trainer.py:232-233 never clears it on auto-reset */

/* action byte formats for mdl_step */
#define MDL_ACTION_TRAINER_INT 0   /* int a: move=['D','L','R','S','U'][a%5], op=a//5 (>=3 -> 0); MAPPO/trainer.py:198-205 */
#define MDL_ACTION_CODES 1         /* move code | op code << 3; move 0..5 = S,L,R,U,D,<other string>; op 0..3 = '0','1','2',<other int> */

typedef struct MdlEngine MdlEngine;

/* Environment(...) constructor arguments (env.py:20-22) + the featurizer /
 * shaping configuration of the trainers (MAPPO/trainer.py:39-64,
 * MAPPO/helper.py:68-70,167-169,271-279, QMIX/config.yaml). */
typedef struct {
    int32_t n_envs;            /* E */
    int32_t n_robots;          /* A, 1..64 */
    int32_t n_packages;        /* P, 1..1024 */
    int32_t max_time_steps;    /* T */
    double move_cost;          /* env.py:21 defaults -0.01 */
    double delivery_reward;    /* 10.0 */
    double delay_reward;       /* 1.0 */
    int32_t tracker_mode;      /* MDL_TRACKER_* */
    double shaping[9];         /* pickup, on_time, late, closer, wasted_pick, wasted_drop, stuck, idle, away */
    int32_t obs_max_time_steps;/* T passed to the feature builders */
    int32_t max_other_robots;  /* MO  (generate_vector_features) */
    int32_t max_packages_obs;  /* MP */
    int32_t max_robots_state;  /* MR  (convert_global_state) */
    int32_t max_packages_state;/* MPs */
    int32_t obs_builder;       /* MDL_OBS_BUILDER_*: which observation kernel mdl_build_obs uses (same outputs) */
    int32_t step_layout;       /* MDL_STEP_LAYOUT_*: how mdl_step maps envs onto wavefronts (same outputs) */
} MdlConfig;

/* MdlConfig.obs_builder.  AUTO: the small builder (flat bit images, one tuple per lane) where it
 * applies (A <= 8, P <= 64, 32-bit sort keys), the general builder otherwise.  GENERIC: always the
 * general builder (any A, P).  Both produce the same floats; GENERIC exists so tests can compare
 * the two on one configuration. */
#define MDL_OBS_BUILDER_AUTO 0
#define MDL_OBS_BUILDER_GENERIC 1

/* MdlConfig.step_layout.  ROWS: a full-batch mdl_step (env_ids NULL) runs four envs per wavefront,
 * one per 16-lane row (A <= 8, P <= 64; mdl_create fails otherwise).  HALVES: two envs per
 * wavefront, one per 32-lane half (A == 16, P <= 128).  WAVE: one env per wavefront always.  AUTO:
 * ROWS where it applies and the batch has at least 7,168 envs, HALVES where it applies and the
 * batch has at least 12,288 envs (the measured crossovers on MI355X), WAVE otherwise.  Subset steps (env_ids),
 * mdl_step_fused, mdl_step_obs and the mailbox step always use one wave per env.  Every layout
 * produces the same state and outputs; the explicit layouts exist so tests can compare them on one
 * configuration. */
#define MDL_STEP_LAYOUT_AUTO 0
#define MDL_STEP_LAYOUT_WAVE 1
#define MDL_STEP_LAYOUT_ROWS 2
#define MDL_STEP_LAYOUT_HALVES 3

/* Create an engine on `device`.  grids: n_maps row-major 0/1 maps packed back
 * to back; map_hw: 2*n_maps (H, W); env_map: E map indices (NULL = all map 0).
 * Replaces Environment.__init__ / load_map (env.py:20-57) and
 * VectorizedEnv.__init__ (MAPPO/env_vectorized.py:2-11) minus seeding. */
int mdl_create(const MdlConfig* cfg, const uint8_t* grids, const int32_t* map_hw, int32_t n_maps,
               const int32_t* env_map, int32_t device, MdlEngine** out);
int mdl_destroy(MdlEngine* eng);

/* RandomState(seed) (env.py:40) for every env -- seeds: E host uint32 -- then
 * the constructor's layout draw (env.py:41).  VectorizedEnv passes seed+i
 * (MAPPO/env_vectorized.py:8-9). */
int mdl_seed(MdlEngine* eng, const uint32_t* seeds, void* stream);

/* Environment.reset() (env.py:81-125) for env_ids[0..n) (device int32; NULL =
 * all E envs, n ignored).  VectorizedEnv.reset(indices) (QMIX/env_vectorized.py:13-21).
 * In MDL_TRACKER_FRESH mode the tracker is implicitly cleared; in
 * MDL_TRACKER_MAPPO_STALE mode it is updated with the reset state, not cleared
 * (MAPPO/trainer.py:232-233); mdl_tracker_clear() clears it explicitly. */
int mdl_reset(MdlEngine* eng, const int32_t* env_ids, int32_t n, void* stream);
int mdl_tracker_clear(MdlEngine* eng, const int32_t* env_ids, int32_t n, void* stream);

/* env_ids (here and in mdl_reset / mdl_tracker_clear / mdl_step_fused / the greedy entry
 * points): a DEVICE int32 array of n ids, each processed once and in parallel, so the ids
 * must be unique and in [0, E); an id outside [0, E) is skipped by the kernels (it cannot
 * touch another env or allocation), duplicates race.  NULL = all E envs in order.  The
 * Python layer checks host-side id lists (list semantics, duplicates refused) before upload.
 *
 * One transition for env_ids[0..n) (NULL = all E in order).
 * Environment.step (env.py:173-306) + compute_shaped_rewards
 * (MAPPO/helper.py:257-369, evaluated with the pre-step tracker) + the
 * tracker update (MAPPO/trainer.py:95-130) + optional reset-on-done
 * (MAPPO/trainer.py:229-257).  actions: device uint8 [n][A] in
 * `action_format`.  Outputs (device, [n], any may be NULL): r_env = the float
 * reward env.step returns (fp64, bit-exact), r_shaped = the float32 value
 * compute_shaped_rewards returns, done = check_terminate (env.py:308-316). */
int mdl_step(MdlEngine* eng, const uint8_t* actions, int32_t action_format, const int32_t* env_ids, int32_t n,
             int32_t auto_reset, double* r_env, float* r_shaped, uint8_t* done, void* stream);

/* mdl_step for all E envs followed by mdl_build_obs(eng, 0, E, ...) of the new state --
 * the trainer's per-step sequence (MAPPO/trainer.py:229-286: env.step, reset on done,
 * tracker update, then convert_observation x A, generate_vector_features x A and
 * convert_global_state of the next state).  Same outputs as the two calls (bit-exact);
 * for A <= 8, P <= 64 they run as ONE kernel that builds the observations from the
 * state the step leaves in registers (no second launch, no state reload), otherwise
 * as the two launches.  The E envs must share one map shape; any output may be NULL. */
int mdl_step_obs(MdlEngine* eng, const uint8_t* actions, int32_t action_format, int32_t auto_reset, double* r_env,
                 float* r_shaped, uint8_t* done, float* actor_map, float* actor_vec, float* critic_map,
                 float* critic_vec, void* stream);

/* One transition of a QMIX episode batch (QMIX/trainer.py:333-526 steps only the envs whose episode
 * is still running): the full batch, row w = env w, the envs sharing one map shape as in mdl_step_obs.
 * active: DEVICE uint8 [E], the caller's, read and updated on the device (no host round trip).
 *   active[e] != 0: exactly mdl_step with auto_reset = 0 on env e (state, fp64 reward, shaped
 *     reward, done, tracker update, episode results: bit for bit), then mdl_build_obs of its new
 *     state into row e of the four observation tensors; filled[e] = 1; active[e] is cleared when
 *     the env is done after the step.
 *   active[e] == 0: nothing of env e is touched; r_env[e] = r_shaped[e] = done[e] = filled[e] = 0
 *     and its rows of the observation tensors are NOT written.
 * The launch steps whatever `active` marks -- it does not check whether an env is past its last
 * step -- and never resets.  r_env / r_shaped / done / filled ([E], device) and the observation
 * pointers may be NULL.  Where mdl_step_obs is one kernel (the small builder, A <= 8, P <= 64)
 * this is one kernel too (an inactive env's wave reads its mask byte and leaves); otherwise a
 * fixed sequence of launches (mask -> id list, the subset step, mask update, the builder over the
 * stepped rows), also without host synchronisation, so either form can be captured in a hipGraph.
 * An engine whose envs mix map shapes is accepted only with all four observation pointers NULL (the
 * step alone, by that fixed sequence: follow it with mdl_build_obs_canvas and the window builders under
 * `filled`); with any observation pointer it fails with a message, as no such tensor has one shape. */
int mdl_step_episode(MdlEngine* eng, const uint8_t* actions, int32_t action_format, uint8_t* active, double* r_env,
                     float* r_shaped, uint8_t* done, uint8_t* filled, float* actor_map, float* actor_vec,
                     float* critic_map, float* critic_vec, void* stream);

/* Bench mode: k_steps consecutive mdl_step calls fused
 * into one launch, each env's state held in registers between steps.  Same
 * results as k_steps mdl_step calls with actions[k] (bit-exact); actions are
 * [k_steps][n][A], r_env / r_shaped / done are [k_steps][n].  Not part of the
 * reference interface: a trainer needs the policy between steps. */
int mdl_step_fused(MdlEngine* eng, const uint8_t* actions, int32_t action_format, const int32_t* env_ids, int32_t n,
                   int32_t k_steps, int32_t auto_reset, double* r_env, float* r_shaped, uint8_t* done, void* stream);

/* Measurement aid (no reference counterpart): the launch floor of mdl_step over n envs -- one
 * launch of an EMPTY kernel with mdl_step's grid, workgroup size, LDS request and kernel-argument
 * layout (so the same preloaded argument registers and kernarg segment).  bench.py replays it the
 * way it replays mdl_step and reports the step's time above this floor.  Touches no state. */
int mdl_step_floor(MdlEngine* eng, int32_t n, void* stream);

/* ---- IDQ / qmix featurizers and IDQ reward shaping ----
 * mdl_build_obs_alt, for envs [env_begin, env_begin+n) sharing one map shape (H, W):
 *   idq_obs    f32 [n][A][6][H][W]       convert_state                IDQ/networks.py:112-217
 *                                        (qmix/networks.py:243-348 is the same function)
 *   qmix_state f32 [n][7][out_h][out_w]  convert_global_state_to_tensor qmix/networks.py:350-468
 *                                        with state_tensor_shape (7, out_h, out_w); the trainers pass (7, H, W)
 * Either pointer may be NULL.  The IDQ / qmix trainers clear their tracker per episode: build the
 * engine with MDL_TRACKER_FRESH for them.
 * mdl_views_alt_features: the same on packed dict views (as mdl_views_features: one map shape per
 * call, records not validated -- see there).
 * mdl_views_idq_reward: reward_shaping (IDQ/networks.py:228-349) per agent, fp64, out[op_offsets[w]+a];
 * ops_are_ints = 0 reproduces IDQ/trainer.py, which passes string ops (so no op branch fires). */
int mdl_build_obs_alt(MdlEngine* eng, int32_t env_begin, int32_t n, float* idq_obs, float* qmix_state, int32_t out_h,
                      int32_t out_w, void* stream);
int mdl_views_alt_features(MdlEngine* eng, const int32_t* views, const int64_t* offsets, int32_t n_views,
                           int32_t max_slots, const int32_t* agent_idx, float* idq_obs, float* qmix_state,
                           int32_t out_h, int32_t out_w, void* stream);
int mdl_views_idq_reward(MdlEngine* eng, const int32_t* prev_views, const int64_t* prev_offsets, int32_t max_slots,
                         const int32_t* cur, const int64_t* cur_offsets, const uint8_t* ops, const int64_t* op_offsets,
                         int32_t ops_are_ints, int32_t n, double* out, void* stream);

/* One IDQ transition's device side, after the step (DQNTrainer.run_episode, IDQ/trainer.py:286-311):
 * reward_shaping (IDQ/networks.py:228-349) per agent and convert_state of the next state, from engine
 * state, for all E envs (one map shape), row e = env e.  reward_shaping reads the state and the tracker
 * from BEFORE the step, which mdl_step has already replaced; what it reads of them is kept in a
 * caller-owned pre-record: a DEVICE buffer of mdl_alt_pre_bytes bytes, 16-byte aligned -- per (env,
 * agent) 16 bytes (the robot word; whether a tracked, waiting, started package starts on the agent's
 * cell; the carried tracked package's target cell and deadline), then int32 t per env.  The engine
 * keeps no hidden state for it: checkpoints, mdl_reset and the step entry points are unaffected.
 *   row_mask != NULL and row_mask[e] == 0: r_idq[e][0..A) = 0 (where actions != NULL); env e's rows
 *     of idq_obs / qmix_state and of the pre-record are NOT written.
 *   otherwise: r_idq[e][a] (f64 [E][A], reward_shaping's accumulation order) from pre[e], the new
 *     robot words, the new t and the op of actions[e][a] (uint8 [E][A], decoded by action_format as
 *     mdl_step does; ops_are_ints = 0 hands over op -1 -- IDQ/trainer.py passes string ops, so only
 *     the stay penalty fires); then pre[e] = the record of the new state, and the observations of the
 *     new state as mdl_build_obs_alt writes them (idq_obs f32 [E][A][6][H][W], qmix_state f32
 *     [E][7][out_h][out_w]; either may be NULL).
 *   actions == NULL ("begin", after a reset): no reward, only the pre-record and the observations.
 * Per step: mdl_step_episode(actions, active, ..., filled, no observations), then
 * mdl_alt_transition(actions, ..., row_mask = filled, ...).  One launch; captures into a hipGraph. */
int mdl_alt_pre_bytes(const MdlEngine* eng, int64_t* bytes);
int mdl_alt_transition(MdlEngine* eng, const uint8_t* actions, int32_t action_format, int32_t ops_are_ints,
                       const uint8_t* row_mask, void* pre, double* r_idq, float* idq_obs, float* qmix_state,
                       int32_t out_h, int32_t out_w, void* stream);

/* The lazy reset that opens a time step of the map-QMIX cycle (QMixTrainer.collect_and_train_cycle,
 * qmix/trainer.py:329-346), for all E envs (one map shape), row e = env e, one launch.  All pointers
 * DEVICE.  done: the caller's uint8 [E], read and updated here.
 *   done[e] != 0, in this order: completed[e] = 1; completed_return[e] = the env's total_reward (the
 *     trainer's env_episode_rewards: the same fp64 sum in the same order); completed_steps[e] = t; the
 *     env's tracker is emptied and Environment.reset() runs (qmix/trainer.py:334-336) -- the engine
 *     state afterwards, the env's MT19937 state included, is what mdl_tracker_clear(ids) followed by
 *     mdl_reset(ids) leaves, in both tracker modes (stale: the reset's own tracker update on the empty
 *     tracker); done[e] = 0; rows e of idq_obs (f32 [E][A][6][H][W]) and qmix_state (f32
 *     [E][7][out_h][out_w]) receive what mdl_build_obs_alt writes for the new state.
 *   done[e] == 0: completed[e] = 0, completed_return[e] = 0.0, completed_steps[e] = 0; nothing else of
 *     env e is read or written, its rows of the two tensors stay as they are.
 * The launch resets what the mask marks; it does not look at t.  Any of completed, completed_return,
 * completed_steps, idq_obs and qmix_state may be NULL.  The buffers must not overlap one another: done
 * and completed in particular are two buffers.  The engine gains no state (checkpoints are unaffected).
 * Captures into a hipGraph. */
int mdl_cycle_begin(MdlEngine* eng, uint8_t* done, uint8_t* completed, double* completed_return,
                    int32_t* completed_steps, float* idq_obs, float* qmix_state, int32_t out_h, int32_t out_w,
                    void* stream);

/* ---- greedy baseline: greedyagent.py batched on the device ----
 * mdl_greedy_init = GreedyAgents() + init_agents(state) for the listed envs (call it right
 * after their reset, as evaluation.py:29-35 does); the first call also builds run_bfs's
 * distance field for every cell of every map (maps of <= 4096 cells).
 * mdl_greedy_actions = one get_actions(state) per listed env (call once per step, before
 * mdl_step), written as MDL_ACTION_CODES bytes [n][A].  Bug-compatible with the reference
 * agent (duplicated t=0 package entries, id-1 list indexing).  After mdl_load_state of a
 * checkpoint without greedy records, only a call without an id list (env_ids == NULL: every env)
 * makes mdl_greedy_actions usable again. */
int mdl_greedy_init(MdlEngine* eng, const int32_t* env_ids, int32_t n, void* stream);
int mdl_greedy_actions(MdlEngine* eng, const int32_t* env_ids, int32_t n, uint8_t* actions, void* stream);

/* mdl_greedy_actions for an episode batch whose running-env mask lives on the device (the greedy
 * loop of evaluation.py:28-47 over E envs at once, with no host round trip): the full batch, row e =
 * env e, actions uint8 [E][A] in MDL_ACTION_CODES.
 * active: DEVICE uint8 [E], the caller's (mdl_step_episode's mask), read and never written.
 *   active[e] != 0: exactly mdl_greedy_actions on env e -- the action bytes and the agent record
 *     afterwards are bit for bit the same.
 *   active[e] == 0: actions[e][0..A) = 0, i.e. ('S', '0'); nothing else of env e is read or written,
 *     its agent record included (get_actions appends the spawns of this t to the record, so a skipped
 *     env's record must stay as it is).  The env's wave reads its mask byte and leaves.
 *   active == NULL: mdl_greedy_actions(eng, NULL, E, actions, stream).
 * Preconditions and errors are mdl_greedy_actions': mdl_greedy_init has run, and after mdl_load_state
 * of a checkpoint without greedy records only mdl_greedy_init without an id list makes it usable
 * again.  Mixed map shapes are allowed.  One launch (mdl_greedy_actions' kernel with the mask
 * pointer), no allocation; captures into a hipGraph. */
int mdl_greedy_actions_masked(MdlEngine* eng, const uint8_t* active, uint8_t* actions, void* stream);

/* What an evaluation reads of each env's episode (evaluation.py:49-51), without mdl_read_state's
 * tables: DEVICE outputs [E], row e = env e, any of them may be NULL.
 *   total_reward f64  the env's total_reward: the same bits mdl_read_state returns
 *   delivered    i32  the number of package slots j < P whose status is delivered
 *                     (sum(1 for p in env.packages if p.status == 'delivered'); == the count of
 *                     status 3 in mdl_read_state's pkgs[e][:][7])
 *   steps        i32  t
 * One launch, one wave per env; touches no state and the engine gains none.  Captures into a hipGraph. */
int mdl_episode_results(MdlEngine* eng, double* total_reward, int32_t* delivered, int32_t* steps, void* stream);

/* The valid-action mask of every robot, from the engine state: avail DEVICE uint8 [E][A][15], 1 =
 * available, in the trainer-int column order (column a = move 'D','L','R','S','U'[a % 5], op a / 5;
 * MAPPO/trainer.py:84-89).  The reference has no counterpart (QMIX/trainer.py:395-397 fills its
 * avail_u with ones); the rule is pinned against env.step (env.py:173-306).  It describes the state
 * the next mdl_step acts on.  For robot i at cell c, prop(m) = the neighbour cell of move m, c for S:
 *   move m is valid:  S always; L/R/U/D iff valid_position(prop(m)) (env.py:197).  Other robots are
 *                     ignored: collisions are resolved inside the step.
 *   op 0 is available with every valid move.
 *   op 1 (pick up) iff the robot carries nothing and a package whose env status is waiting starts
 *                     at c or at prop(m) (env.py:264-274; waiting implies start_time <= t)
 *   op 2 (drop)    iff the robot carries package id and that package's target is c or prop(m)
 *                     (env.py:277-292) -- both cells count, because the robot ends the step on one
 *                     of them and which one depends on the other robots.
 *   An invalid move has all three of its columns 0.
 * So an action is masked exactly when, whatever the other robots do, the step equals the step with
 * its reduction: the invalid move replaced by S, then the op unavailable under that move by 0.
 * Column 3 ('S', op 0) is always 1.  Env truth (status bits, package table): the same in both
 * tracker modes.
 * active: DEVICE uint8 [E] (mdl_step_episode's mask), read and never written, or NULL.  An env whose
 *   byte is 0 gets all ones (the reference's placeholder) and nothing of it is loaded; with NULL every
 *   env is computed, a done one too.
 * One launch, one wave per env; touches no state and the engine gains none.  Captures into a hipGraph. */
int mdl_avail_actions(MdlEngine* eng, const uint8_t* active, uint8_t* avail, void* stream);

/* ---- dict-API mailbox: the per-call path of Environment.step / reset on single envs ----
 * Environment.step (env.py:173-306) and VectorizedEnv.step / reset(indices) (QMIX/env_vectorized.py:13-37)
 * return Python dicts per call, so their cost is the host <-> GPU round trip, not the step.  The mailbox
 * is ONE engine-owned host allocation, fine-grained and mapped into the device: the caller writes action
 * codes (and env ids) into it, the step kernel reads them from there, an export kernel writes the touched
 * envs' rows and a completion word into it, and the call spins on that word (no device staging buffers,
 * no copy-engine transfers, no stream synchronisation).  Row w of every output = the w-th env of the call
 * (ids[w] with use_ids, else env w).  The pointers stay valid until mdl_destroy; the outputs of a call
 * are overwritten by the next one.  Calls are synchronous (they return once the rows are in the mailbox). */
typedef struct {
    int32_t* seq;          /* completion word (device-written) */
    uint8_t* codes;        /* in:  [E][A] MDL_ACTION_CODES bytes */
    int32_t* ids;          /* in:  [E] env ids of the call (unique, in [0, E)) */
    double* r_env;         /* out: [E] env.step's reward (fp64) */
    float* r_shaped;       /* out: [E] compute_shaped_rewards (engine tracker) */
    uint8_t* done;         /* out: [E] */
    int32_t* robots;       /* out: [E][A][3] (row, col, carrying), 0-indexed */
    int32_t* pkgs;         /* out: [E][P][8] as mdl_read_state */
    int32_t* t;            /* out: [E] */
    double* total_reward;  /* out: [E] */
    int32_t* rterms;       /* out: [E] reward terms the step added: MDL_RTERM_* bits (0 after a reset) */
} MdlMailbox;
#define MDL_RTERM_MOVE 1    /* a move cost (env.py:256) */
#define MDL_RTERM_ONTIME 2  /* an on-time delivery reward (env.py:288) */
#define MDL_RTERM_LATE 4    /* a late delivery reward (env.py:291) */
/* Allocates the mailbox on first use (E-sized sections) and returns its pointers. */
int mdl_mailbox(MdlEngine* eng, MdlMailbox* out);
/* mdl_step(codes, MDL_ACTION_CODES, ids or all E) on the mailbox's inputs, then the rows of those envs. */
int mdl_mail_step(MdlEngine* eng, int32_t n, int32_t use_ids, int32_t auto_reset, void* stream);
/* mdl_reset of those envs (Environment.reset, env.py:81-125), then their rows. */
int mdl_mail_reset(MdlEngine* eng, int32_t n, int32_t use_ids, void* stream);
/* The rows of those envs only (after other engine calls on `stream`). */
int mdl_mail_export(MdlEngine* eng, int32_t n, int32_t use_ids, void* stream);

/* Host-mapped scratch for the helper-compatible calls on single dicts (convert_observation,
 * generate_vector_features, convert_global_state, compute_shaped_rewards: MAPPO/helper.py:6-369):
 * the caller packs the view records into it and passes its addresses to mdl_views_* as both the
 * inputs and the outputs -- the kernels read and write host memory directly -- then calls
 * mdl_host_wait, which returns once everything queued on `stream` before it has finished (a
 * one-wave kernel publishes a completion word the call spins on).  mdl_host_arena returns at least
 * `bytes` of it (16-byte aligned; a larger request replaces the arena, so earlier addresses die). */
int mdl_host_arena(MdlEngine* eng, int64_t bytes, void** out);
int mdl_host_wait(MdlEngine* eng, void* stream);
/* mdl_views_features / mdl_views_shaped_reward with their inputs and outputs in the arena, and
 * synchronous: the launch's own waves publish the arena's completion word when the last of them
 * has written its outputs (no mdl_host_wait launch behind it), and the call returns once it has
 * seen it.  `stream` need not be the caller's compute stream: nothing on the device waits for or
 * on these calls.  (The helper functions of marl_gpu.helper call these from C, _mdl_pack.) */
int mdl_host_views_features(MdlEngine* eng, const int32_t* views, const int64_t* offsets, int32_t n_views,
                            int32_t max_slots, const int32_t* agent_idx, int32_t T, int32_t MO, int32_t MP,
                            int32_t MR, int32_t MPs, float* obs, float* vec, float* gmap, float* gvec, void* stream);
int mdl_host_views_shaped_reward(MdlEngine* eng, const int32_t* prev_views, const int64_t* prev_offsets,
                                 int32_t max_slots, const int32_t* cur, const int64_t* cur_offsets,
                                 const uint8_t* actions, const int64_t* act_offsets, const double* g, int32_t n,
                                 const double* consts, float* out, void* stream);
/* One view / one transition with its inputs in the caller's host memory (any: they are copied
 * into the kernel's arguments at launch, so the wave reads them without round trips to host
 * memory) and its outputs in the arena; synchronous as above.  rec: one view record (layout of
 * mdl_views_features) of `words` <= MDL_VIEW_INLINE_WORDS words.  For the shaped reward the
 * previous view, the current record and the action codes together must fit that capacity
 * (prev_words + cur_words + ceil(n_actions / 4)); n_actions >= the view's robots.  Larger
 * inputs take the arena entries above.  The shaped reward comes back beside the completion word,
 * so `out` may be any host memory.  The single-call paths of marl_gpu.helper. */
#define MDL_VIEW_INLINE_WORDS 768
int mdl_host_view_features(MdlEngine* eng, const int32_t* rec, int32_t words, int32_t agent_index, int32_t T,
                           int32_t MO, int32_t MP, int32_t MR, int32_t MPs, float* obs, float* vec, float* gmap,
                           float* gvec, void* stream);
int mdl_host_view_shaped_reward(MdlEngine* eng, const int32_t* prev_view, int32_t prev_words, const int32_t* cur,
                                int32_t cur_words, const uint8_t* actions, int32_t n_actions, double g,
                                const double* consts, float* out, void* stream);

/* ---- checkpoint of the engine state ----
 * A versioned host blob: a 56-byte header (magic "MDLSTATE", version, E, A, P, T, tracker mode,
 * map fingerprint) then every state buffer (robots, packages, state words, env records,
 * MT19937 states, tracker data, episode results).  Loading it into an engine of the same
 * configuration resumes every env's stream exactly, RNG included; any other engine refuses it.
 * save / load are synchronous on `stream`; the buffer is host memory. */
int mdl_state_bytes(MdlEngine* eng, int64_t* bytes);
int mdl_save_state(MdlEngine* eng, void* host_buf, int64_t bytes, void* stream);
int mdl_load_state(MdlEngine* eng, const void* host_buf, int64_t bytes, void* stream);

/* ---- rollout glue: keeps MAPPO/trainer.py:133-290 on the device ---- */

/* Categorical(logits=...).sample() and .log_prob() (MAPPO/trainer.py:141-143) for n_rows rows of
 * n_actions float32 logits (row-major, contiguous).  Inverse CDF of softmax(logits) on a
 * Philox4x32-10 uniform keyed by (seed, offset, row): deterministic for a given (seed, offset),
 * independent of launch shape; a caller advances `offset` once per call.  actions: uint8 [n_rows]
 * (the trainer-int action, ready for mdl_step); log_probs: float32 [n_rows] or NULL.
 * log_prob = (l_a - max) - log(S) in float32, S the sequential float32 sum of expf(l_i - max) and log(S)
 * the fp64 logarithm of S rounded once to float32 (logf was 1.05 ulp off at S = 57, which a row of 57
 * equal logits returned as it came: tests/test_gpu_rollout_shapes.py). */
int mdl_sample_actions(const float* logits, int64_t n_rows, int32_t n_actions, uint64_t seed, uint64_t offset,
                       uint8_t* actions, float* log_probs, void* stream);

/* The same draw with the offset read on the device: offset = *offset_dev + offset_add, so a
 * captured hipGraph of a whole rollout replays with fresh offsets (MAPPO/trainer.py:141-143:
 * each rollout samples new actions).  Identical results to mdl_sample_actions at that offset. */
int mdl_sample_actions_dev(const float* logits, int64_t n_rows, int32_t n_actions, uint64_t seed,
                           const uint64_t* offset_dev, uint64_t offset_add, uint8_t* actions, float* log_probs,
                           void* stream);

/* mdl_sample_actions / mdl_sample_actions_dev over the softmax restricted to each row's available
 * actions.  avail: DEVICE uint8 [n_rows][n_actions] (non-zero = available, mdl_avail_actions' rows),
 * or NULL = every action available.  The same Philox keying and the same inverse CDF, with the
 * unavailable actions left out of the maximum, of the sum and of the running sum: an unavailable
 * action has probability exactly 0 and is never returned, and log_probs is the log of the
 * renormalised probability, (l_a - max_avail) - log(sum_avail exp(l_i - max_avail)).  A row with no
 * available action gets action 0 and log-prob -inf.  With avail NULL or all non-zero, actions and
 * log-probs are bit for bit mdl_sample_actions' at the same (seed, offset). */
int mdl_sample_actions_avail(const float* logits, const uint8_t* avail, int64_t n_rows, int32_t n_actions,
                             uint64_t seed, uint64_t offset, uint8_t* actions, float* log_probs, void* stream);
int mdl_sample_actions_avail_dev(const float* logits, const uint8_t* avail, int64_t n_rows, int32_t n_actions,
                                 uint64_t seed, const uint64_t* offset_dev, uint64_t offset_add, uint8_t* actions,
                                 float* log_probs, void* stream);

/* Epsilon-greedy action selection over Q-values (QMIX/trainer.py:298-319), the library's random
 * stream in place of torch's.  q: float32 [n_rows][n_actions]; avail: uint8 of the same shape
 * (non-zero = available) or NULL = every action available; actions: uint8 [n_rows].  Per row:
 *   (x0, x1, x2, x3) = Philox4x32-10(counter = (offset lo, offset hi, row lo, row hi),
 *                                    key = (seed lo, seed hi))      -- mdl_sample_actions's keying
 *   explore  iff  float(x0 >> 8) * 2^-24 < epsilon   (a float32 compare: epsilon = 0 never
 *                                                     explores, epsilon = 1 always does)
 *   exploring row: the k-th available action in index order (k from 0),
 *                  k = (uint64(x1) * n_avail) >> 32
 *   any other row: best = the first available action; then every later available action i, in
 *                  index order, replaces it iff q[i] > q[best], or q[best] is a NaN and q[i] is
 *                  not -- the lowest index among the available actions with the largest q; a NaN
 *                  never wins over a number
 *   a row with no available action gets 0.
 * Deterministic for a given (seed, offset) and independent of the launch shape; a caller advances
 * `offset` once per call.  The _dev form reads epsilon = *epsilon_dev and offset = *offset_dev +
 * offset_add on the device, so a captured episode replays with fresh values; identical results to
 * the host form at the same values. */
int mdl_select_actions_eps(const float* q, const uint8_t* avail, int64_t n_rows, int32_t n_actions, float epsilon,
                           uint64_t seed, uint64_t offset, uint8_t* actions, void* stream);
int mdl_select_actions_eps_dev(const float* q, const uint8_t* avail, int64_t n_rows, int32_t n_actions,
                               const float* epsilon_dev, uint64_t seed, const uint64_t* offset_dev,
                               uint64_t offset_add, uint8_t* actions, void* stream);
/* The same selections (bit-identical actions), which also report the rows that explored: explored uint8
 * [n_rows] = 1 where the row explored (float(x0 >> 8) * 2^-24 < epsilon and it had an available action),
 * else 0.  qmix/trainer.py:251-260 keeps an exploring agent's hidden state. */
int mdl_select_actions_eps_mark(const float* q, const uint8_t* avail, int64_t n_rows, int32_t n_actions,
                                float epsilon, uint64_t seed, uint64_t offset, uint8_t* actions, uint8_t* explored,
                                void* stream);
int mdl_select_actions_eps_mark_dev(const float* q, const uint8_t* avail, int64_t n_rows, int32_t n_actions,
                                    const float* epsilon_dev, uint64_t seed, const uint64_t* offset_dev,
                                    uint64_t offset_add, uint8_t* actions, uint8_t* explored, void* stream);

/* *counter += value on the device (stream-ordered; advances offset_dev inside a graph). */
int mdl_counter_add(uint64_t* counter, uint64_t value, void* stream);

/* One step's appends to IDQ's per-transition replay buffer (the buffer.add calls of
 * IDQ/trainer.py:304-311 on ReplayBuffer.add, IDQ/networks.py:63-79), needing no engine: for every env
 * with filled[e] != 0, in env order, and every agent a in order, one row (obs[e][a], actions[e][a],
 * reward[e][a], next_obs[e][a], done[e]) goes to ring slot ptr; then ptr = (ptr + 1) % capacity and
 * size = min(size + 1, capacity).  All pointers DEVICE: filled, done uint8 [E]; obs, next_obs f32
 * [E][A][row_floats]; actions uint8 [E][A]; reward f64 [E][A] (stored rounded once to float32, as the
 * reference's float32 array does); cursor int64 [2] = (ptr, size), read and advanced on the device (no
 * host round trip); the ring: ring_obs, ring_next_obs f32 [capacity][row_floats], ring_action int64,
 * ring_reward f32, ring_done uint8 [capacity]; rank_scratch int32 [E + 3] (the envs' ranks among the
 * filled ones, then the filled count and the step's first slot).  Two launches: a one-workgroup prefix
 * sum over `filled` that also advances the cursor, and the copy, one wave per filled env (16-byte
 * vectors where row_floats % 4 == 0 and the four row pointers are 16-byte aligned).  A step with more
 * rows than `capacity` leaves its last `capacity` rows, each written once, as the sequential adds do.
 * E <= MDL_REPLAY_MAX_ENVS (the prefix sum is one workgroup's loop); a larger E is refused. */
#define MDL_REPLAY_MAX_ENVS 65536
int mdl_replay_append(const uint8_t* filled, int32_t E, int32_t A, int64_t row_floats, const float* obs,
                      const float* next_obs, const uint8_t* actions, const double* reward, const uint8_t* done,
                      int64_t capacity, int64_t* cursor, float* ring_obs, float* ring_next_obs, int64_t* ring_action,
                      float* ring_reward, uint8_t* ring_done, int32_t* rank_scratch, void* stream);

/* One step's appends to the qmix/ trainer's joint replay buffer (ReplayBuffer.add, qmix/networks.py:155-198,
 * called for every env of the step: qmix/trainer.py:380-389), needing no engine.  In env order, ring slot
 * (ptr + e) % capacity receives state[e] and next_state[e] (f32, state_floats each), obs[e] and
 * next_obs[e] (f32, A * obs_floats each), actions[e][0..A) (uint8 -> int64), reward[e] (f64 -> f32,
 * rounded once) and done[e] (uint8); then ptr = (ptr + E) % capacity and size = min(size + E, capacity).
 * All pointers DEVICE; cursor int64 [2] = (ptr, size).  The ring: ring_state, ring_next_state f32
 * [capacity][state_floats]; ring_obs, ring_next_obs f32 [capacity][A * obs_floats]; ring_action int64
 * [capacity][A]; ring_reward f32 and ring_done uint8 [capacity].  Of a step with E > capacity only the
 * last `capacity` rows are written, each once.  Two launches, so that the cursor is never read and
 * advanced in one grid: the copy, one wave per env, reads it (16-byte vectors where state_floats and
 * A * obs_floats are multiples of 4 and the eight row pointers are 16-byte aligned); a one-thread
 * launch then advances it.  Both capture into a hipGraph.  The step's rows must not overlap the ring
 * (state and next_state, or obs and next_obs, may be one buffer: they are only read). */
int mdl_replay_append_joint(int32_t E, int32_t A, int64_t state_floats, int64_t obs_floats, const float* state,
                            const float* next_state, const float* obs, const float* next_obs, const uint8_t* actions,
                            const double* reward, const uint8_t* done, int64_t capacity, int64_t* cursor,
                            float* ring_state, float* ring_next_state, float* ring_obs, float* ring_next_obs,
                            int64_t* ring_action, float* ring_reward, uint8_t* ring_done, void* stream);

/* Generalised advantage estimation exactly as MAPPO/trainer.py:266-276 computes it in float32
 * (same operation order): rewards, values, dones [T][n] (dones uint8), next_value [n];
 * gamma = float32(GAMMA), gamma_lambda = float32(GAMMA * GAE_LAMBDA) with the product in double.
 * Writes advantages and returns (= advantages + values) [T][n]. */
int mdl_gae(const float* rewards, const float* values, const float* next_value, const uint8_t* dones, int32_t T,
            int64_t n, float gamma, float gamma_lambda, float* advantages, float* returns, void* stream);

/* Observation builders for envs [env_begin, env_begin+n), which must share one
 * map shape (H, W), from the current state + tracker:
 *   actor_map  f32 [n][A][6][H][W]          convert_observation       MAPPO/helper.py:6-66
 *   actor_vec  f32 [n][A][6+5MO+5MP+1]      generate_vector_features  MAPPO/helper.py:68-165
 *   critic_map f32 [n][4][H][W]             convert_global_state[0]   MAPPO/helper.py:167-198
 *   critic_vec f32 [n][6MR+7MPs+1]          convert_global_state[1]   MAPPO/helper.py:199-255
 * Any output pointer may be NULL. */
int mdl_build_obs(MdlEngine* eng, int32_t env_begin, int32_t n, float* actor_map, float* actor_vec,
                  float* critic_map, float* critic_vec, void* stream);

/* The element type of the four observation tensors of mdl_build_obs_as / mdl_step_obs_as.  F16 (IEEE
 * binary16) and BF16: every element is the float32 value mdl_build_obs writes, rounded once to
 * nearest-even (ties to even, signed zeros and fp16 subnormals kept) -- bit for bit the float32
 * tensor converted on the host. */
#define MDL_OBS_F32 0
#define MDL_OBS_F16 1
#define MDL_OBS_BF16 2

/* mdl_build_obs with the outputs' element type `dtype` (MDL_OBS_*; the tensors' shapes are
 * mdl_build_obs's, their elements 2 bytes for the half types, 2-byte aligned at least).  MDL_OBS_F32
 * is mdl_build_obs itself; an unknown dtype fails with a message. */
int mdl_build_obs_as(MdlEngine* eng, int32_t env_begin, int32_t n, int32_t dtype, void* actor_map, void* actor_vec,
                     void* critic_map, void* critic_vec, void* stream);

/* mdl_step_obs with the observations' element type `dtype`.  MDL_OBS_F32 is mdl_step_obs itself (its
 * one-launch form where that applies); the half types always run mdl_step's launch followed by the
 * builder's (there is no fused half kernel).  Rewards, done and the engine's state do not depend on
 * dtype. */
int mdl_step_obs_as(MdlEngine* eng, const uint8_t* actions, int32_t action_format, int32_t auto_reset, double* r_env,
                    float* r_shaped, uint8_t* done, int32_t dtype, void* actor_map, void* actor_vec,
                    void* critic_map, void* critic_vec, void* stream);

/* Robot-centred actor-map windows (no reference counterpart: a crop of convert_observation's tensor).
 * For radius R = `radius` in [1, MDL_EGO_MAX_RADIUS] and K = 2R + 1, robot a on 0-based cell (r, c):
 *   actor_ego [n][A][6][K][K],  ego[a][ch][i][j] = actor_map[a][ch][r - R + i][c - R + j]
 * where that cell lies inside the env's map (actor_map: exactly what mdl_build_obs writes for the same
 * state, tracker mode and clock); outside the map channel 0 (obstacles) is 1.0 -- an off-map cell cannot
 * be entered -- and channels 1-5 are 0.0.  Channel 1 is therefore a single 1.0 at (R, R).  The carried
 * package's target (channel 5) may lie outside the window, which is then all zero in that channel; the
 * actor vector still carries the target.  `dtype` (MDL_OBS_*) is the element type, the half types the
 * float32 values rounded once (values are 0 or 1).  The output shape does not depend on the map, so the
 * range is checked against [0, E) only and may cross map shapes.  Asynchronous on `stream`, no host
 * round trip.  A radius outside [1, MDL_EGO_MAX_RADIUS] or an unknown dtype fails with a message. */
#define MDL_EGO_MAX_RADIUS 15
int mdl_build_obs_ego(MdlEngine* eng, int32_t env_begin, int32_t n, int32_t radius, int32_t dtype, void* actor_ego,
                      void* stream);

/* mdl_build_obs_ego under a row mask, for the episode loops (after mdl_step_episode, with its `filled`).
 * rows: DEVICE uint8 [E], indexed by ENV ID (rows[e] for env e of [env_begin, env_begin + n), not by the
 * output row e - env_begin); non-zero = build.  The output row of env e is the unmasked call's
 * (actor_ego + (e - env_begin) * A * 6 * K * K elements); rows of unmarked envs are not written, not one
 * byte -- they keep what the caller's buffer held.  The mask is read on the device by the launch itself:
 * the call is asynchronous on `stream` with no host round trip, so it can be captured in a hipGraph.
 * Every other check and meaning is mdl_build_obs_ego's.  rows == NULL fails with a message: the unmasked
 * entry point exists for that case. */
int mdl_build_obs_ego_masked(MdlEngine* eng, int32_t env_begin, int32_t n, const uint8_t* rows, int32_t radius,
                             int32_t dtype, void* actor_ego, void* stream);

/* Robot-centred windows of the IDQ / map-QMIX agent observation (no reference counterpart: a crop of
 * convert_state's tensor, IDQ/networks.py:112-217 == qmix/networks.py:243-348).  For radius R = `radius` in
 * [1, MDL_EGO_MAX_RADIUS] and K = 2R + 1, robot a on 0-based cell (r, c):
 *   idq_ego [n][A][6][K][K] float32,  idq_ego[a][ch][i][j] = idq_obs[a][ch][r - R + i][c - R + j]
 * where that cell lies inside the env's map (idq_obs: exactly what mdl_build_obs_alt writes for the same
 * state, tracker mode and clock); outside the map channel 0 is 1.0 and channels 1-5 are 0.0.  Channel 4 is
 * therefore a single 1.0 at (R, R); channel 1 holds the same float32 urgency bits as the full tensor; a
 * carrying robot has all-zero channels 1 and 2; the carried id's target (channel 5) may lie outside the
 * window.  The output is float32 only: the urgency plane would not survive a half type exactly, and the
 * replay rings (mdl_replay_append*) take float rows -- there is no half form of these windows.
 * rows: NULL (every env of the range), or DEVICE uint8 [E] indexed by ENV ID (rows[e] for env e of
 * [env_begin, env_begin + n), not by the output row e - env_begin); non-zero = build.  The output row of
 * env e is idq_ego + (e - env_begin) * A * 6 * K * K elements either way; rows of unmarked envs are not
 * written, not one byte.  The mask is read on the device by the launch itself.
 * The output shape does not depend on the map, so the range is checked against [0, E) only and may cross
 * map shapes (mdl_build_obs_alt refuses that).  Asynchronous on `stream`, no host round trip: the call can
 * be captured in a hipGraph.  n == 0 succeeds and launches nothing.  A radius outside
 * [1, MDL_EGO_MAX_RADIUS], a null idq_ego with n > 0 or an LDS slice that does not fit fail with a message
 * and leave the engine usable.  mdl_step_episode, the dict-API helpers and the views entry points
 * (mdl_views_alt_features) have no window form. */
int mdl_build_obs_alt_ego(MdlEngine* eng, int32_t env_begin, int32_t n, const uint8_t* rows /* NULL: every env */,
                          int32_t radius, float* idq_ego, void* stream);

/* The critic's (or mixer's) observations of envs of several map shapes at once: the critic map on a fixed
 * canvas, and the two vector observations, whose row sizes do not depend on the map.
 * For a canvas (Hc, Wc) = (canvas_h, canvas_w), anchored at the map's top-left cell, and an env of an H x W map:
 *   critic_canvas [n][4][Hc][Wc],  canvas[ch][i][j] = critic_map[ch][i][j]   for i < H and j < W
 *                                                   = 1.0 in channel 0, 0.0 in channels 1-3 elsewhere
 * (critic_map: exactly what mdl_build_obs writes for the same state, tracker mode and clock; an off-map
 * cell reads as an obstacle, the windows' rule).  With (Hc, Wc) == (H, W) it is critic_map byte for byte.
 *   actor_vec [n][A][6+5MO+5MP+1], critic_vec [n][6MR+7MPs+1]: each env's rows bit for bit what
 * mdl_build_obs_as writes for that env, normalised by its own map's H and W.
 * dtype: MDL_OBS_*, a half element being the float32 value rounded once.  Each output pointer may be NULL.
 * The range is checked against [0, E) only and may cross map shapes.  The canvas is one launch over the
 * range; the vectors take the builders' launch once per run of consecutive same-shape envs of the range.
 * rows: NULL (every env of the range), or DEVICE uint8 [E] indexed by ENV ID (rows[e] for env e, not by
 * the output row e - env_begin); non-zero = build.  The output rows of env e are at row e - env_begin
 * either way; rows of unmarked envs are not written, not one byte, in all three tensors.
 * Asynchronous on `stream`, no host round trip: the call can be captured in a hipGraph.  n == 0 succeeds
 * and launches nothing.  No cropping: a canvas smaller than a map of the range in either dimension fails
 * with a message, as do Hc or Wc outside [1, 255], Hc * Wc > MDL_MAX_CELLS, an unknown dtype and an LDS
 * slice that does not fit; the engine stays usable. */
int mdl_build_obs_canvas(MdlEngine* eng, int32_t env_begin, int32_t n, const uint8_t* rows /* NULL: every env */,
                         int32_t dtype, int32_t canvas_h, int32_t canvas_w, void* actor_vec, void* critic_canvas,
                         void* critic_vec, void* stream);

/* State snapshot into caller DEVICE buffers (async on `stream`).  Any pointer may be NULL.
 *   robots   int32 [E][A][3]  (row, col, carrying), 0-indexed
 *   pkgs     int32 [E][P][8]  (sr, sc, tr, tc, start_time, deadline, id, status 0 None/1 waiting/2 in_transit/3 delivered)
 *   t        int32 [E];  total_reward f64 [E]
 *   tracker  int32 [E][P][4]  per id 1..P: (present, in_transit, order, _) ; data rows in tracker_data int32 [E][P][6]
 * Backs the dict view of Environment.get_state (env.py:127-147). */
int mdl_read_state(MdlEngine* eng, int32_t* robots, int32_t* pkgs, int32_t* t, double* total_reward,
                   int32_t* tracker, int32_t* tracker_data, void* stream);

/* Helper-compatible builders on arbitrary state dicts ("views"): the same
 * device code as mdl_build_obs / the fused shaping, fed from a packed int32
 * record per view instead of engine state.  View record layout (int32):
 *   [0] t  [1] A  [2] n_slots  [3] map index
 *   then A x (row, col, carrying)           0-indexed robot rows (state['robots'] minus 1)
 *   then n_slots x (id, status 1|2, sr, sc, tr, tc, start_time, deadline)  tracker in dict order
 * views: device int32 blob; offsets: device int64 [n_views] record starts;
 * max_slots: the largest n_slots of any record (sizes the LDS slice).
 * Robot and package cells must lie inside the view's map.
 * agent_idx: device int32 [n_views] (may be out of range -> reference's
 * early-return outputs).  Outputs per view: obs [6][H][W], vec [6+5MO+5MP+1],
 * gmap [4][H][W], gvec [6MR+7MPs+1] (NULL to skip).  T/MO/MP/MR/MPs are call
 * arguments here.  Replaces convert_observation / generate_vector_features /
 * convert_global_state called on dicts (MAPPO/helper.py:6-255).
 *
 * One map shape per call: all views of one mdl_views_features (or
 * mdl_host_views_features, mdl_views_alt_features) call must name maps of the
 * same (H, W); the maps themselves may differ.  Row w of obs, gmap and idq_obs
 * starts at w * rows * H * W of the view's own map (rows = 6, 4, 6), so views
 * of different shapes in one call would write overlapping rows.  Views of
 * several shapes go into one call per shape.  mdl_views_shaped_reward and
 * mdl_views_idq_reward have no per-shape output and may mix shapes freely.
 *
 * View records are NOT validated: they live on the device (or in the arena)
 * and the library never reads them on the host.  A map index outside the
 * engine's maps, a cell outside the view's map, n_slots > max_slots, A >
 * MDL_MAX_ROBOTS or an offset outside the blob makes the kernel read or
 * write out of bounds.  The caller guarantees all of these. */
int mdl_views_features(MdlEngine* eng, const int32_t* views, const int64_t* offsets, int32_t n_views,
                       int32_t max_slots, const int32_t* agent_idx, int32_t T, int32_t MO, int32_t MP, int32_t MR, int32_t MPs,
                       float* obs, float* vec, float* gmap, float* gvec, void* stream);

/* compute_shaped_rewards (MAPPO/helper.py:257-369) on dict inputs: prev view
 * record (state + tracker_prev as above), current robots int32 [A][3]
 * (0-indexed) and time, actions uint8 [A] in MDL_ACTION_CODES, global reward
 * (fp64).  cur: device int32 blob, cur_offsets: int64 [n] (record = [t, A,
 * then A x 3]); actions: uint8 blob with act_offsets int64 [n]; g: f64 [n];
 * consts: host double[9] (NULL = engine's).  Output: f32 [n]. */
int mdl_views_shaped_reward(MdlEngine* eng, const int32_t* prev_views, const int64_t* prev_offsets, int32_t max_slots,
                            const int32_t* cur, const int64_t* cur_offsets, const uint8_t* actions,
                            const int64_t* act_offsets, const double* g, int32_t n, const double* consts,
                            float* out, void* stream);

/* Host-only (no GPU needed): the distance-rank table the feature sorts use.
 * out[(dr+H-1)*(2W-1) + dc+W-1] = rank of the fp64 key (dr/H)**2 + (dc/W)**2
 * (CPython float_pow -> libm pow) among all distinct keys of the map shape;
 * equal doubles share a rank.  out holds (2H-1)*(2W-1) entries.  This is the
 * order of others.sort / pkgs.sort in MAPPO/helper.py:139,158. */
int mdl_rank_table(int32_t H, int32_t W, uint16_t* out);

/* Introspection */
int mdl_get_config(const MdlEngine* eng, MdlConfig* out);
/* The step layout (MDL_STEP_LAYOUT_WAVE, _ROWS or _HALVES) mdl_step launches for a call over n envs
 * (use_ids = 0: the full batch, n ignored as in mdl_step; use_ids = 1: an env_ids subset of n,
 * always WAVE) -- the engine's own decision, the one mdl_step takes. */
int mdl_step_layout(const MdlEngine* eng, int32_t n, int32_t use_ids, int32_t* layout);
/* The layout of the last mdl_step launch on this engine (0 before the first one). */
int mdl_last_step_layout(const MdlEngine* eng, int32_t* layout);
/* The symbol (as rocprof reports it, e.g. "mdl::k_step<true, 1, false, 5>") of the kernel mdl_step
 * launches in `layout` (WAVE / ROWS / HALVES), or, with with_obs, of mdl_step_obs's step launch (its fused
 * step + observation kernel where it applies).  NUL-terminated into out[cap]. */
int mdl_step_kernel_name(const MdlEngine* eng, int32_t layout, int32_t with_obs, char* out, int32_t cap);
/* The symbol (as rocprof reports it, e.g. "mdl::k_obs_small<true, false>") of the observation builder
 * mdl_build_obs (dtype = MDL_OBS_F32) or mdl_build_obs_as (MDL_OBS_F16 / _BF16) launches: the small
 * builder k_obs_small<ST, RL> / k_obs_small_h<ST, RL, BF> (RL: the distance-rank table staged in LDS)
 * or the general one, k_obs<ST> / k_obs_h<ST, BF>; ST: the stale tracker.  It comes from the selection
 * the builder launch itself runs.  NUL-terminated into out[cap]. */
int mdl_obs_kernel_name(const MdlEngine* eng, int32_t dtype, char* out, int32_t cap);
int mdl_obs_dims(const MdlEngine* eng, int32_t* actor_vec_dim, int32_t* critic_vec_dim);
const char* mdl_last_error(void);
const char* mdl_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MDL_ENGINE_H */
