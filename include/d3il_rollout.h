/* d3il_rollout.h - C ABI of libd3il_rollout.so, the MI355X-native batched replacement for the D3IL
 * evaluation env.step() path.  Plain C, plain pointers and sizes; no torch types.
 *
 * The reference has no FFI layer: its operator boundary is the Gym-style Python protocol of the task
 * envs.  Each entry point below names the reference interface it replaces (paths relative to
 * /root/reference); the Python mirror of those classes lives in d3il_amd/envs and d3il_amd/simulation.
 *
 * Conventions
 *  - every function returns 0 on success, a negative D3IL_E* code on failure; d3il_last_error() gives
 *    the message of the calling thread's last failure.
 *  - the library owns all device memory it hands out through d3il_get_buffers(); the caller owns the
 *    action buffer.  Device pointers are valid until d3il_destroy().
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Kernels are only enqueued;
 *    the caller synchronises (PyTorch: pass torch.cuda.current_stream().cuda_stream so that
 *    agent.predict() consumes observations in place without extra synchronisation).
 *  - one host thread per handle; calls on one handle are not re-entrant.
 *  - there is NO CPU fallback: d3il_create fails with D3IL_ENODEVICE when no HIP device is usable.
 *
 * State layout (device, f64): structure-of-arrays [D3IL_STATE_F64][stride], stride = n_envs rounded up
 * to 64, field order D3IL_STATE_*; one lane owns one environment, loads/stores are coalesced.
 */
#ifndef D3IL_ROLLOUT_H
#define D3IL_ROLLOUT_H
#include <stddef.h>
#include <stdint.h>
#include "d3il_model_blob.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct d3il_handle_s* d3il_handle;

enum {
  D3IL_OK = 0, D3IL_EINVAL = -1, D3IL_EBLOB = -2, D3IL_ENODEVICE = -3, D3IL_EHIP = -4, D3IL_EUNSUPPORTED = -5,
  D3IL_ESTATE = -6, D3IL_ERCCL = -7
};

/* Tasks (task_id of d3il_create; the enum itself is D3IL_TASK_* in d3il_model_blob.h: 0 Avoiding, 1 Pushing, 2 Sorting, 3 Stacking, 4 Aligning, 5 Inserting) and
 * their shapes:
 *   task      reference env (environments/d3il/envs/...)            action (device f64, row-major)              obs f32   contexts f64     state rows
 *   Avoiding  gym_avoiding/envs/avoiding.py ObstacleAvoidanceEnv    [n][7] desired TCP x y z qw qx qy qz        [n][2]    none             42
 *   Pushing   gym_pushing/envs/pushing.py Block_Push_Env            [n][7] same                                 [n][8]    [n][14]          91
 *   Sorting   gym_sorting/envs/sorting.py Sorting_Env (2 / 4 boxes) [n][7] same                                 [n][2+3b] [n][7 b]         42+13b+(9+6b)+2
 *   Stacking  gym_stacking/envs/stacking.py CubeStacking_Env        [n][8] 7 desired joint positions + gripper   [n][12]   [n][21]          94
 *                                                                   command (open iff > 0.075, stacking.py:337-346)
 *   Aligning  gym_aligning/envs/aligning.py Robot_Push_Env          [n][7] as Avoiding (the harness commands z)  [n][17]   [n][14]          77
 *   Inserting gym_inserting/envs/gate_insertion.py Gate_Insertion_Env [n][7] as Avoiding                          [n][11]   [n][21]          110
 */

/* f64 state fields per environment, in SoA order */
enum {
  D3IL_STATE_QPOS = 0,    /* 9: 7 arm joints, 2 fingers */
  D3IL_STATE_QVEL = 9,    /* 9 */
  D3IL_STATE_BIAS = 18,   /* 7: qfrc_bias of the last forward pass (gravity compensation is one sub-step stale) */
  D3IL_STATE_TCP = 25,    /* 3: TCP xpos of the last forward pass (what MjRobot.receiveState reads) */
  D3IL_STATE_IK_Q = 28,   /* 7: CartPosQuatImpedenceController.old_q */
  D3IL_STATE_IK_QD = 35,  /* 7: CartPosQuatImpedenceController.old_des_joint_vel */
  D3IL_STATE_F64 = 42,
  /* Pushing appends: per cube pos[3] quat[4] vel[6] (qpos/qvel of its free joint: linear velocity in world axes, angular
   * velocity in body axes), then the constraint solver's warm start qacc[21] (cube1, cube2, arm), then the two task rows info['mean_distance'] and reward
   * (pushing.py:335-407) - d3il_buffers.info_f64 points AT these two rows (a view of the state buffer, no copy).  91 rows since the task runs on the generic
   * engine (library version 2; 89 before: a version-1 checkpoint lacks the task rows).  Size state buffers from d3il_buffers.state_rows, not from a constant. */
  D3IL_PUSH_STATE_BOX = 42, D3IL_PUSH_STATE_WARM = 68, D3IL_PUSH_STATE_TASK = 89, D3IL_PUSH_STATE_F64 = 91,
  /* Sorting-4 (sorting.py): per cube pos[3] quat[4] vel[6] in the order red_1, red_2, blue_1, blue_2, the solver's warm start
   * qacc[33] (cubes, arm), then the task state of Sorting_Env as two words stored as doubles: word 0 = mode[6], two bits each
   * (value + 1), | mode_step << 12;  word 1 = min_inds[6], three bits each (sorting.py:405-411, 460-507) */
  D3IL_SORT_STATE_BOX = 42, D3IL_SORT_STATE_WARM = 94, D3IL_SORT_STATE_TASK = 127, D3IL_SORT_STATE_F64 = 129,
  /* Stacking (stacking.py; robot panda_invisible.xml, joint-space controller: no IK rows): rows 0..27 as above up to the TCP (qpos 9, qvel 9,
   * qfrc_bias 7, TCP 3), then per box pos[3] quat[4] vel[6] in the order red, green, blue (D3IL_STACK_STATE_BOX + 13 k), then the
   * constraint solver's warm start qacc[27] (box 0, box 1, box 2, arm 9).  The task state of CubeStacking_Env (order in which the boxes
   * reached the target zone, stacking.py:395-419) lives in the flag word (D3IL_SFLAG_*). */
  D3IL_STACK_STATE_BOX = 28, D3IL_STACK_STATE_WARM = 67, D3IL_STACK_STATE_F64 = 94,
  /* Aligning (gym_aligning/envs/aligning.py; the rod robot, Cartesian controller: rows 0..41 as for Avoiding): the free compound body
   * (robot_push_box.xml: plate + four walls) pos[3] quat[4] vel[6] as MuJoCo's free joint holds them (body origin, body-frame angular velocity),
   * the solver's warm start qacc[15] (box 6 - in centre-of-mass coordinates -, arm 9), the target pose pos[3] quat[4] of the context
   * (aligning.py:107-122; it only enters observation, reward and success).  Flag word: the Pushing bits (mode + 1 in D3IL_PFLAG_MODE_MASK: 0 / 1 =
   * rod inside / outside the walls, aligning.py:288-312; WARM_VALID, OFF_TABLE, CON_OVERFLOW) and D3IL_SFLAG_HAND_NEAR. */
  D3IL_ALIGN_STATE_BOX = 42, D3IL_ALIGN_STATE_WARM = 55, D3IL_ALIGN_STATE_TARGET = 70, D3IL_ALIGN_STATE_F64 = 77,
  /* Inserting (gate_insertion.py; the Sorting layout with three cubes push_box1..3 = red, green, blue): cubes 13 each, warm start qacc[27], then the task
   * state of Gate_Insertion_Env: word 0 = number of letters in `modes` | letter k (1 r, 2 g, 3 b) << (2 + 2 k) (gate_insertion.py:411-432); word 1 =
   * info['mean_distance'] of the last step, a double (:434-446).  mode buffer: info['mode'] (mode_dict code once all three letters are in, else 0,
   * :386-409) | number of letters << 3 (one / two / three_box_success = that number >= 1 / 2 / 3).  Contexts: 3 x (x, y, z = 0, quat) (:94-113). */
  D3IL_INS_STATE_BOX = 42, D3IL_INS_STATE_WARM = 81, D3IL_INS_STATE_TASK = 108, D3IL_INS_STATE_F64 = 110
};
/* bits of the per-environment u32 flag word */
enum {
  D3IL_FLAG_MODE_MASK = 0x1FF,       /* 9 sticky mode bits, avoiding.py:173-202 */
  D3IL_FLAG_L1 = 1 << 9, D3IL_FLAG_L2 = 1 << 10, D3IL_FLAG_L3 = 1 << 11,
  D3IL_FLAG_TERMINATED = 1 << 12, D3IL_FLAG_SUCCESS = 1 << 13, D3IL_FLAG_ROD_CONTACT = 1 << 14,
  D3IL_FLAG_IK_VALID = 1 << 15,
  D3IL_FLAG_SOLVER_FAIL = 1 << 16,   /* a solver did not converge, or the action held NaN / Inf (the step then ran on a fixed safe set-point and the episode is terminated) */
  D3IL_FLAG_MULTI_CONTACT = 1 << 17,
  /* Pushing reuses TERMINATED / SUCCESS / IK_VALID / SOLVER_FAIL and replaces the low bits: */
  D3IL_PFLAG_FIRST_MASK = 0x7,       /* first_visit + 1 (pushing.py:341-377) */
  D3IL_PFLAG_MODE_MASK = 0x38,       /* (mode + 1) << 3 */
  D3IL_PFLAG_WARM_VALID = 1 << 6,
  D3IL_PFLAG_CON_OVERFLOW = 1 << 18, /* more contacts than the solver holds (24) in some sub-step */
  D3IL_PFLAG_OFF_TABLE = 1 << 19,    /* a cube left the modelled part of the table */
  D3IL_PFLAG_LINK_NEAR = 1 << 20,    /* Pushing / Sorting / Inserting with d3il_set_link_guard: a bounding capsule of a robot collision hull this engine does not collide
                                        (link0 .. link7, hand, fingers) came within the guard margin of a cube or a static box at the end of some env step of the
                                        episode; the same bit and meaning as D3IL_SFLAG_HAND_NEAR */
  /* Stacking reuses TERMINATED / SUCCESS / SOLVER_FAIL / CON_OVERFLOW (more than 32 contacts) / OFF_TABLE and replaces the low bits: */
  D3IL_SFLAG_MODE_MASK = 0xFF,       /* order code n | c0 << 2 | c1 << 4 | c2 << 6: n boxes have reached the target zone, c_i = colour (0 r, 1 g, 2 b) of the
                                        i-th one (info['mode'] = "rgb"[c0] + ... , stacking.py:395-419); also what buf.mode holds */
  D3IL_SFLAG_WARM_VALID = 1 << 8,    /* the warm-start rows hold the accelerations of the previous sub-step (the gripper command is re-derived from the action every step, so
                                        RobotBase.grasp_flag needs no bit) */
  D3IL_SFLAG_HAND_NEAR = 1 << 20     /* a box came within the bounding box of a robot collision geom this engine does not evaluate */
};

typedef struct d3il_buffers {
  int32_t n_envs, stride, obs_dim, action_dim;
  float* obs;            /* [n_envs][obs_dim] f32, what get_observation() returns (avoiding.py:117-119, pushing.py:255-280) */
  uint8_t* done;         /* [n_envs] result of is_finished() of the last step (gym_env_wrapper.py:124-137) */
  uint8_t* success;      /* [n_envs] info[1] (avoiding.py:171) */
  uint16_t* mode;        /* [n_envs] Avoiding: 9-bit mode encoding, bit i = mode_encoding[i] (info[0]); Pushing: info['mode'] as int16 (-1..3);
                            Sorting: int(np.packbits(mode)[0]); Stacking: order code (D3IL_SFLAG_MODE_MASK) */
  double* state;         /* [state_rows][stride] */
  uint32_t* flags;       /* [stride] */
  int32_t* step_count;   /* [stride] env_step_counter */
  double* policy_des;    /* [3][stride] random-policy harness state: desired x, y and fixed z */
  double* info_f64;      /* [n_info_f64][stride] extra f64 step outputs; Pushing: info['mean_distance'], reward (pushing.py:335-407); Stacking: info['mean_distance'] */
  int32_t n_info_f64, state_rows;   /* state_rows: f64 state fields per environment (42 Avoiding, 91 Pushing, 129 Sorting-4, 94 Stacking, 77 Aligning, 110 Inserting) */
  uint8_t* last_reset;   /* [n_envs] environments reset by the last d3il_auto_reset (non-zero): per-lane harness / agent state re-latches from it */
} d3il_buffers;

/* Replaces: env construction + scene.start() (avoiding.py:52-92, core/Scene.py:95-108,
 * mj_scene_parser.py:36-53 building MjModel).  model_blob is a d3il_model_blob. */
int d3il_create(int task_id, int n_envs, int device_id, const void* model_blob, size_t blob_len, d3il_handle* out);
int d3il_destroy(d3il_handle h);

/* Replaces the part of env.start() that survives it: robot.init_qpos (avoiding.py:121-166).
 * The offline IK that produces init_qpos is host-side, cold (d3il_amd/controllers/offline_ik.py). */
int d3il_start(d3il_handle h, const double* init_qpos7);

/* Replaces env.reset() (avoiding.py:248-262).  env_mask: device u8[n_envs] (non-zero = reset that env) or
 * NULL for all.  contexts: NULL for Avoiding; Pushing (pushing.py:461-483 with random=False): device f64 [n_envs][14] =
 * per env 2 x (x, y, z, qw, qx, qy, qz) written into the cubes' qpos as BlockContextManager.set_context does (z = 0);
 * Sorting-4 (sorting.py:545-575): device f64 [n_envs][28] = 4 x (x, y, z = 0.05, quat), red boxes first (sorting.py:121-187).
 * Sorting outputs: obs f32 [n_envs][14] (TCP xy, then x, y, tan(yaw) per box), mode = int(np.packbits(mode[:4])[0]).
 * Stacking (stacking.py:449-481 with random=False): device f64 [n_envs][21] = 3 x (x, y, z = 0, qw, qx, qy, qz) for the red, green and blue box
 * (BlockContextManager.set_context, stacking.py:99-125); fingers opened before the reset sub-step (:474).  Stacking outputs: obs f32 [n_envs][12] =
 * (x, y, z, tan(yaw)) per box (stacking.py:228-277), mode = the order code of D3IL_SFLAG_MODE_MASK, info_f64[0] = info['mean_distance']. */
int d3il_reset(d3il_handle h, const uint8_t* env_mask, const double* contexts, void* stream);

/* Replaces env.step(action) (avoiding.py:168-171 over gym_env_wrapper.py:45-100): n_substeps fused physics
 * sub-steps.  actions: device f64[n_envs][7] = desired TCP (x, y, z, qw, qx, qy, qz), the array the harness
 * builds at avoiding_sim.py:64-66.  Stacking (stacking.py:331-393, 30 sub-steps): device f64[n_envs][8] = 7 desired joint positions of the
 * joint-space PD law + the gripper command (open iff > 0.075, else close_fingers), the array the harness builds at stacking_sim.py:99-106. */
int d3il_step(d3il_handle h, const double* actions, void* stream);

int d3il_get_buffers(d3il_handle h, d3il_buffers* out);

/* Golden replay / checkpointing: copies the SoA state + flags + step counters to/from host memory
 * (state: f64[state_rows][n_envs] packed with stride n_envs; flags u32[n_envs]; steps i32[n_envs]; any of the three may be NULL).
 * state_rows = the row count the CALLER's buffer was sized for; it must equal d3il_buffers.state_rows of the handle, otherwise nothing is copied
 * and D3IL_EINVAL is returned (a buffer sized from a stale constant cannot be overrun, a checkpoint of another layout cannot be loaded). */
int d3il_get_state(d3il_handle h, double* state, int32_t state_rows, uint32_t* flags, int32_t* steps);
int d3il_set_state(d3il_handle h, const double* state, int32_t state_rows, const uint32_t* flags, const int32_t* steps);

/* Device-side random-policy harness of BASELINE config 2, counterpart of the rollout loop in
 * simulation/avoiding_sim.py:51-66 with agent.predict := U(-0.01, 0.01)^2 (Philox4x32-10, key = seed,
 * counter = (env_offset + env, t)).  policy_begin latches des = TCP xyz for masked envs (avoiding_sim.py:53-54);
 * policy_action advances des_xy and writes actions[n_envs][7]. */
int d3il_policy_begin(d3il_handle h, const uint8_t* env_mask, void* stream);
int d3il_policy_action(d3il_handle h, uint64_t seed, uint64_t env_offset, uint32_t t, double* actions, void* stream);

/* Vectorised-env auto-reset: every environment whose `done` flag is set is reset (as d3il_reset with mask = done; Pushing /
 * Sorting: with the context of that environment's last d3il_reset), the harness re-latches its desired pose (policy_des := TCP,
 * avoiding_sim.py:53-54, pushing_sim.py:69-70, sorting_sim.py:120-121), episode_counts (device i64[2], may be NULL for
 * Pushing / Sorting) += {finished, successful} episodes, and buf.last_reset marks the environments that were reset.
 * Counterpart of starting the next trajectory in the rollout loops (avoiding_sim.py:45-54, pushing_sim.py:43-66). */
int d3il_auto_reset(d3il_handle h, int64_t* episode_counts_device, void* stream);

/* Policy-side helper (batched policy adapters): causal self-attention of the reference's DiffusionGPT
 * (agents/models/beso/agents/diffusion_agents/k_diffusion/score_gpts.py:15-80) for its short token sequences, fused: qkv f32
 * [B * T][3 H D] (query | key | value per token), out f32 [B * T][H D]; softmax over the keys j <= i, scores scaled by
 * 1 / sqrt(D).  Device pointers, T <= 32, D <= 32; needs no handle.  (D a multiple of 4 and both pointers 16-byte aligned: 16-byte loads; anything else takes the
 * scalar instantiation, same sums in the same order.)  A NaN in a query, key or value makes NaN exactly the outputs whose masked softmax is NaN - the queries
 * at and behind that key of that (sequence, head), query 0 with its single key included; no other (sequence, head) changes. */
int d3il_attention_causal_f32(const float* qkv, float* out, int B, int T, int H, int D, void* stream);

/* Policy-side helper: LayerNorm over the last dimension (torch.nn.LayerNorm semantics) for rows of 4 .. 128 floats (a multiple of 4):
 * the transformer of the reference's BESO policy normalises [B * T][120] activations 13 times per denoising call
 * (score_gpts.py:83-115, :353).  x, y f32 [rows][C]; 16-byte aligned device pointers.  A NaN / Inf in a row makes that row NaN and no other. */
int d3il_layernorm_f32(const float* x, const float* weight, const float* bias, float* y, long rows, int C, float eps, void* stream);
/* Fused transformer MLP of the batched DiffusionGPT (score_gpts.py:83-115: x + fc2(GELU(fc1(h))), h = ln2(x)) on the f32 matrix cores:
 * out[rows][C] = x + b2 + W2 GELU(W1 h + b1).  w_packed = both weight matrices in the per-chunk LDS order of the kernel (d3il_amd/policies.py
 * pack_mlp_weights; H / 16 chunks of 4096 floats).  Built for C = 120, H = 480 (D3IL_EUNSUPPORTED otherwise); all device pointers, 16-byte aligned. */
int d3il_mlp_gelu_residual_f32(const float* h, const float* x, const float* w_packed, const float* b1, const float* b2, float* out, long rows, int C, int H, void* stream);
/* The same with the LayerNorm in front fused in (h = the block's residual stream x itself, ln_weight / ln_bias / ln_eps of ln2; NULL weights = no LayerNorm). */
int d3il_mlp_ln_gelu_residual_f32(const float* h, const float* ln_weight, const float* ln_bias, float ln_eps, const float* x, const float* w_packed, const float* b1, const float* b2,
                                  float* out, long rows, int C, int H, void* stream);
/* out[rows][N] = (LayerNorm)(xin)[rows][120] W^T + bias (+ resid[rows][N]) on the f32 matrix cores: the 120-input linear layers of the DiffusionGPT block
 * (query | key | value as ONE product with N = 360 after ln1; the attention output projection with the residual, N = 120).  w_packed = W [N][120] in the
 * kernel's tile order (d3il_amd/policies.py pack_linear120_weights: ceil(N / 16) tiles of 2048 floats).  ln_weight NULL = no LayerNorm; resid NULL = none. */
int d3il_linear120_f32(const float* xin, const float* ln_weight, const float* ln_bias, float ln_eps, const float* w_packed, const float* bias, const float* resid, float* out,
                       long rows, int N, void* stream);

/* The same two products on the f16 matrix cores with SPLIT operands (csrc/policy_f16x3.h): every f32 operand x = xh + 2^-11 xl as two f16 numbers (22 of the 24
 * significant bits), w x = wh xh + 2^-11 (wh xl + wl xh) in f32 accumulators - three v_mfma_f32_16x16x32_f16 per f32 product instead of sixteen f32-MFMA issue slots.
 * Agreement with an f64 reference is that of an f32 FMA chain (tests/test_policies_f16x3.py); operands saturate at +-65504.  w_packed: f16 halves in the kernels' tile
 * order (d3il_amd/policies.py pack_mlp_weights_f16x3: 16 stages of 2048 x 16 bytes; pack_linear120_weights_f16x3: an even number of tiles of 512 x 16 bytes).
 * The saturation is silent, and it turns a NaN / Inf operand into a finite number too (+-Inf into +-65504, NaN into -65504: tests/test_gpu_f16x3_edges.py), unless the
 * range / NaN guard below is on.  Every pointer the kernels read or write by 16-byte vectors has to be 16-byte aligned (D3IL_EINVAL otherwise, before any launch):
 * h | x | w_packed | b1 | b2 | out of the MLP, xin | w_packed | bias | resid | out of the linear layer. */
int d3il_mlp_ln_gelu_residual_f16x3(const float* h, const float* ln_weight, const float* ln_bias, float ln_eps, const float* x, const void* w_packed, const float* b1, const float* b2,
                                    float* out, long rows, int C, int H, void* stream);
int d3il_linear120_f16x3(const float* xin, const float* ln_weight, const float* ln_bias, float ln_eps, const void* w_packed, const float* bias, const float* resid, float* out,
                         long rows, int N, void* stream);
/* The attention half of a DiffusionGPT block (score_gpts.py:35-80 CausalSelfAttention, 103-107 Block.forward first line) in one launch:
 * out = x + proj(causal_attention(LayerNorm(x) Wqkv' + b_qkv)) + b_proj for n_seq sequences of T <= 16 tokens x 120 features, 6 heads; one wave per sequence,
 * q | k | v never leave the CU.  w_packed: the 24 tiles of the packed (query | key | value) weight followed by the 8 tiles of the packed projection weight
 * (policies.pack_linear120_weights_f16x3 of both, concatenated).  out must not alias x. */
int d3il_attn_half_f16x3(const float* x, const float* ln_weight, const float* ln_bias, float ln_eps, const void* w_packed, const float* b_qkv, const float* b_proj, float* out,
                         long n_seq, int T, int n_head, int C, void* stream);
/* The whole block chain of a 72-wide transformer trunk (n_embd 72, 4 heads of 18, hidden 288: the Avoiding / Aligning / Pushing / Sorting-2 configs) in one launch
 * (csrc/policy_trunk72.h), split-f16 products as above: for l < n_layer
 *     x = x + proj_l(causal_attention_4heads(LayerNorm1_l(x) Wqkv_l' + bqkv_l)) + bproj_l;   x = x + W2_l GELU(W1_l LayerNorm2_l(x) + b1_l) + b2_l     (exact GELU).
 * x and out are f32 [n_seq][T][72]; one wave owns floor(16 / T) whole sequences, the residual stream never leaves the CU.  out must not alias x.
 * w_packed: f16, n_layer x 28 stages x 768 vectors of 16 bytes (policies.pack_trunk72_weights), lane = 16 g + i, p = 0 the high half, 1 the low half times 2^11,
 * zero beyond the matrices:
 *   stages 0 .. 6, vector ((u * 3 + s) * 2 + p) * 64 + lane = Wqkv_p[16 (2 stage + u) + i][32 s + 8 g + e], Wqkv = query | key | value rows, 216 x 72;
 *   stages 7 .. 9 the same form with the projection (stage - 7 for stage);
 *   stage 10 + 2 k (k < 9), vector ((tile * 3 + s) * 2 + p) * 64 + lane = W1_p[32 k + 16 tile + i][32 s + 8 g + e];
 *   stage 11 + 2 k, vector (t * 2 + p) * 64 + lane = W2_p[16 t + i][32 k + 16 (e >> 2) + 4 g + (e & 3)], t < 6.
 * vec: f32, n_layer x 936: ln1.weight | ln1.bias | b_qkv (216) | b_proj | ln2.weight | ln2.bias | b1 (288) | b2.  ln_eps: the one epsilon of all 2 n_layer LayerNorms.
 * Built for 1 <= T <= 16, 1 <= n_layer <= 8, n_seq >= 1: D3IL_EUNSUPPORTED otherwise; D3IL_EINVAL for a null pointer, one that is not 16-byte aligned, or out == x;
 * both answered before any launch.  Under the range / NaN guard below the split sites per layer are the LayerNorm1 row, the attention output row, the LayerNorm2 row
 * and the GELU outputs; a row is counted at most once per counter and LAUNCH (all layers); a non-finite operand makes its row and the later tokens of its own
 * sequence NaN and changes no other sequence, those that share its tile included.
 * (The return type stands on a line of its own: tests/test_capi_signatures.py pins the number of `int d3il_*_f16x3(` lines; tests/test_capi_signatures5.py reads this form.) */
int
d3il_gpt_trunk72_f16x3(const float* x, const void* w_packed, const float* vec, float ln_eps, float* out, long n_seq, int T, int n_layer, void* stream);
/* Sampling head of the batched Behaviour-Transformer policy (policies.BeTPolicy; bet_agent.py:359-372, latent_generators/mingpt.py:155-186, k_means.py:111-138) in one
 * launch, f32 throughout.  Per row: x = LayerNorm(h); logit_v = w_head[v] . x (v < V); p = exp(logit - max), S = sum p, c = inclusive prefix sums; u = u_in[row] or
 * 24 bits of Philox4x32-10 with key = seed and counter = (env_offset + row, *t_device, a tag word other than the 0 of the random-policy harness), so 0 <= u <= 1 - 2^-24;
 * bin = min(#{v : c_v <= u S}, V - 1); off_a = w_head[V + bin A + a] . x; actions[row][a] = clamp(centers[bin][a] + off_a, lo_a, hi_a) scale_a + shift_a.
 * h [rows][C] (the last block's output, before ln_f), w_head [V (1 + A)][C] row-major as in the reference's state dict, centers [V][A], lo / hi / scale / shift [A],
 * t_device: DEVICE u32 read by the kernel (a captured graph draws fresh numbers when its owner advances the word between replays); u_in, u_out [rows], probs [rows][V]
 * may be NULL; bins i32 [rows].  A row with a NaN / Inf in h gives bins = -1 and NaN in every action component.  Built for V = 64, C <= 128 (a multiple of 4),
 * 1 <= A <= 8: D3IL_EUNSUPPORTED otherwise, answered before any launch.  h and w_head 16-byte aligned. */
int d3il_bet_head_f32(const float* h, const float* ln_weight, const float* ln_bias, float ln_eps, const float* w_head, const float* centers, const float* lo, const float* hi,
                      const float* scale, const float* shift, uint64_t seed, uint64_t env_offset, const uint32_t* t_device, const float* u_in, float* actions, int32_t* bins,
                      float* u_out, float* probs, long rows, int C, int V, int A, void* stream);
/* Everything between two block chains of the batched DDPM-GPT sampler (policies.DDPMGPTPolicy; ddpm_agent.py:213-274, gc_diffusion.py:117-216 around
 * diffusion_models.py DiffusionTransformerNetwork) in one launch, f32 throughout.  k = T - 1 .. 0 are the reverse steps, k = T the init mode.  For environment n and
 * window position j < W: z = LayerNorm(hk[n][j]); eps_a = w_pred[a] . z + b_pred[a]; x0_a = clamp(sched[k][0] x_a - sched[k][1] eps_a, lo_a, hi_a);
 * mean_a = sched[k][2] x0_a + sched[k][3] x_a; x'_a = mean_a + sched[k][4] noise_a (k = 0: x' = mean_a, nothing is drawn).  k > 0: x[n][j] = x',
 * xbuf[n][2 + 2 j][c] = sum_a w_aemb[c][a] x'_a + bias_pos[j][c] and xbuf[n][0] = temb[k - 1]; k = 0: actions[n][a] = clamp(x'_a, lo_a, hi_a) scale_a + shift_a at
 * j = len[n] - 1.  Init mode: x' = noise (hk is not read and may be NULL), bad is cleared.  Positions j >= len[n]: x' = 0, the token is bias_pos[j].
 * noise_a = noise_in[n][j][a] when given (the [n_env][W][A] slice of THIS chain index), otherwise Box-Muller (u1 = ((r0 >> 8) + 1) 2^-24, u2 = (r1 >> 8) 2^-24,
 * sqrt(-2 ln u1) (cos, sin)(2 pi u2); r2, r3 likewise) on Philox4x32-10 with key = seed and counter = (env_offset + n, *t_device, 0x44470000 | k << 8 | j << 1 | q),
 * component a = 4 q + m.  hk [n_env][W][C], w_pred [A][C], w_aemb [C][A] (nn.Linear weights as they are), bias_pos [W][C], temb [T][C], sched [T][5], lo / hi (scaled
 * space) / scale / shift [A], len i64 [n_env] (clamped to 1 .. W), t_device: DEVICE u32, x [n_env][W][A] (in / out), xbuf [n_env][2 W + 1][C], noise_out
 * [n_env][W][A] may be NULL.  bad i32 [n_env]: sticky from the init launch on - set by a NaN / Inf in a valid hidden row, normalised row or iterate; at k = 0 such an
 * environment gets NaN in every action component.  Built for C <= 128 (a multiple of 4), 1 <= A <= 8, 1 <= W <= 16, 1 <= T <= 255: D3IL_EUNSUPPORTED otherwise,
 * answered before any launch. */
int d3il_ddpm_gpt_step_f32(const float* hk, const float* ln_weight, const float* ln_bias, float ln_eps, const float* w_pred, const float* b_pred, const float* w_aemb,
                           const float* bias_pos, const float* temb, const float* sched, const float* lo, const float* hi, const float* scale, const float* shift,
                           const int64_t* len, uint64_t seed, uint64_t env_offset, const uint32_t* t_device, const float* noise_in, float* x, float* xbuf, float* actions,
                           int32_t* bad, float* noise_out, long n_env, int C, int A, int W, int T, int k, void* stream);
/* Everything between two block chains of the batched BESO sampler (policies.BESONativePolicy; beso_agent.py:316-443, gc_sampling.py:107-114 and 217-256 around
 * score_wrappers.py GCDenoiser and score_gpts.py DiffusionGPT; sampler euler_ancestral, linear noise schedule, no goals) in one launch, f32 throughout, in the
 * reference's order of operations.  i = 0 .. S - 1 are the sampling steps, i = -1 the init mode.  For environment n and window position j < W:
 * z = LayerNorm(hk[n][j]); net_a = w_pred[a] . z + b_pred[a]; den_a = coef[i][1] net_a + coef[i][0] x_a; d_a = (x_a - den_a) coef[i][2]; x'_a = x_a + d_a coef[i][3];
 * i < S - 1: x'_a += coef[i][4] noise_a, x[n][j] = x', xbuf[n][2 + 2 j][c] = sum_a w_aemb[c][a] (coef[i][5] x'_a) + bias_pos[j][c] and xbuf[n][0] = semb[i + 1];
 * i = S - 1 (nothing is drawn): a_new = clamp(x'_a, lo_a, hi_a) at j = len[n] - 1, actions[n][a] = a_new scale_a + shift_a, and a_new is pushed onto the action ring
 * a_hist[n] in place (entries move down by one, a_new becomes the last).  Init mode (hk is not read and may be NULL; bad is cleared): x'[j] = a_hist[n][(W - 1) -
 * (len[n] - 1) + j] for j < len[n] - 1, x'[len[n] - 1] = sigma_max noise, tokens with c_in0 and semb[0].  Positions j >= len[n]: x' = 0, the token is bias_pos[j].
 * coef [S][6] = (c_skip, c_out, 1 / s_from, s_down - s_from, s_up, c_in of the NEXT sigma) of the Karras preconditioner and the ancestral step, built on the host.
 * noise_a = noise_in[n][j][a] when given (the [n_env][W][A] slice of THIS draw; the init mode reads row j = 0 only), otherwise Box-Muller normals as
 * d3il_ddpm_gpt_step_f32 on Philox4x32-10 with key = seed and counter = (env_offset + n, *t_device, 0x42530000 | draw << 8 | j << 1 | q), component a = 4 q + m;
 * draw 0 with j = 0 is the init draw (one per environment), draw i + 1 the one of step i.  hk [n_env][W][C], w_pred [A][C], w_aemb [C][A] (nn.Linear weights as they
 * are), bias_pos [W][C], semb [S][C], lo / hi (scaled space) / scale / shift [A], len i64 [n_env] (clamped to 1 .. W), t_device: DEVICE u32, x [n_env][W][A] (in /
 * out), xbuf [n_env][2 W + 1][C], a_hist [n_env][W - 1][A] (newest entry last; may be NULL when W = 1), noise_out [n_env][W][A] may be NULL.  bad i32 [n_env]: sticky
 * from the init launch on - set by a NaN / Inf in a valid hidden row, normalised row or iterate; at i = S - 1 such an environment gets NaN in every action component
 * and in the ring entry it pushes.  Built for C <= 128 (a multiple of 4), 1 <= A <= 8, 1 <= W <= 16, 1 <= S <= 254: D3IL_EUNSUPPORTED otherwise, answered before
 * any launch.  (No _f32 suffix: capi.SIGNATURES2 holds this entry.) */
int d3il_beso_step(const float* hk, const float* ln_weight, const float* ln_bias, float ln_eps, const float* w_pred, const float* b_pred, const float* w_aemb,
                   const float* bias_pos, const float* semb, const float* coef, float sigma_max, float c_in0, const float* lo, const float* hi, const float* scale,
                   const float* shift, const int64_t* len, uint64_t seed, uint64_t env_offset, const uint32_t* t_device, const float* noise_in, float* x, float* xbuf,
                   float* a_hist, float* actions, int32_t* bad, float* noise_out, long n_env, int C, int A, int W, int S, int i, void* stream);
/* The whole inference of the batched Implicit-BC policy (policies.IBCPolicy; ibc_agent.py:248-286, samplers/langevin_mcmc.py:129-163,236-286, ebms.py:21-51) in one
 * launch, f32 throughout: per environment S = 64 samples, K Langevin iterations on the energy network E([state | x]) (ResidualMLPNetwork, Mish, one output) with the
 * analytic gradient, then a categorical draw from softmax(-E) of the final samples.  x_a starts at x0_in[n][s][a] or lo_a + u (hi_a - lo_a); iteration k:
 * g = dE/dx, d_a = clamp(coef[k][0] g_a + coef[k][1] noise_scale z_a, -clip_a, clip_a), x_a = clamp(x_a - d_a, lo_a, hi_a) with z = noise_in[k][n][s] or Box-Muller
 * normals; then p_s = exp(-(E_s - min E)), c = inclusive prefix sums, pick = min(#{s : c_s <= u c_63}, 63) with u = u_in[n] or a Philox uniform, and
 * actions[n][a] = x[pick][a] scale_a + shift_a.  Random numbers: Philox4x32-10, key = seed, counter = (env_offset + n, *t_device, 0x49420000 | kind << 14 | k << 8 |
 * s << 2 | q) with kind 0 = start point, 1 = noise, 2 = draw; component a = 4 q + m takes word m; uniforms (r >> 8) 2^-24, normals as d3il_ddpm_gpt_step_f32.
 * state [n_env][obs_dim] (scaled); w_in .. b_out: policies.pack_resmlp_weights of the network (input row = [state | action]); wT_blocks: the same packing of the
 * TRANSPOSED square layers, in the same order; wT_in_act: the action columns of the input layer as a 16-row output-style tile (row a = W_in[:, obs_dim + a]);
 * coef [K][2] = (f32(step / 2), f32(step)) (may be NULL when K = 0); lo / hi (scaled space) / clip / scale / shift [A]; t_device: DEVICE u32.  x0_in [n_env][S][A], noise_in [K][n_env][S][A],
 * u_in [n_env] and x_final [n_env][S][A], energies [n_env][S], x0_out, noise_out, u_out (what was used) may be NULL; picks i32 [n_env].  K = 0: the energies and the
 * pick of the start points.  An environment with a NaN / Inf in its state row, a start point, a gradient, an iterate or a final energy gets picks = -1 and NaN in
 * every action component; no other environment changes.  Built for hidden 128 / 256, 0 <= n_blocks <= 4, obs_dim + A <= 28, 1 <= A <= 8, S = 64, 0 <= K <= 63:
 * D3IL_EUNSUPPORTED otherwise, answered before any launch.  Packed arrays 16-byte aligned. */
int d3il_ibc_langevin_f32(const float* state, const float* w_in, const float* b_in, const float* w_blocks, const float* b_blocks, const float* w_out, const float* b_out,
                          const float* wT_blocks, const float* wT_in_act, const float* coef, float noise_scale, const float* lo, const float* hi, const float* clip,
                          const float* scale, const float* shift, uint64_t seed, uint64_t env_offset, const uint32_t* t_device, const float* x0_in, const float* noise_in,
                          const float* u_in, float* actions, int32_t* picks, float* x_final, float* energies, float* x0_out, float* noise_out, float* u_out, long n_env,
                          int obs_dim, int A, int hidden, int n_blocks, int S, int K, void* stream);
/* One step of the batched VAE-ACT policy (policies.ACTPolicy; act_agent.py:207-239 around act_vae.py:389-445, ActVAE.forward without actions) in one launch, f32
 * throughout.  Persistent per-environment state on the device: counter i32 [n_env] and chunk [n_env][T][A] (already clamped and inverse-scaled).  An environment with
 * counter == T (or outside 0 .. T) is due: z = latent_in[n] or 32 Philox uniforms; the encoder runs on [W_s state + pos[0], W_z z + pos[1]] (causal mask for T >= 2, as
 * the reference slices it; LayerNorm with weight only, eps 1e-5; exact GELU), the decoder on the T query embeddings (x + proj(causal self-attention(ln1 x) +
 * cross-attention(ln1 x, encoder output)), x + mlp(ln2 x), final LayerNorm, action head); chunk[n][t][a] = clamp(head, lo_a, hi_a) scale_a + shift_a and counter = 0.
 * Every environment then emits actions[n] = chunk[n][counter] and stores counter + 1.  A workgroup (16 environments) without a due environment runs no network;
 * an environment's result never depends on which of its neighbours are due.  Random numbers: Philox4x32-10, key = seed, counter = (env_offset + n, *t_device,
 * 0x41430000 | q), q < 8; latent component 4 q + m = (word m >> 8) 2^-24.  state [n_env][obs_dim] (scaled); w_in, tab, enc_w, enc_v, dec_w, dec_v, head_w:
 * policies.pack_act_weights of the network (fragment order [To][t][lane (g, i)][r] = W[16 To + i][16 t + 4 g + r]; per layer the matrices q k v proj fc1 fc2 /
 * q k v cq ck cv proj fc1 fc2 and the vectors ln1 ln2, the biases in the same order, b1 b2; tab = pos [2][64] | query_embed [8][64] | encoder ln | decoder ln | head
 * bias [16]); lo / hi (scaled space) / scale / shift [A]; t_device: DEVICE u32, read only.  latent_in [n_env][32] and latent_out [n_env][32] (what was used; written
 * for due environments only) may be NULL.  A due environment with a NaN / Inf in its state row or in a head output gets NaN in its whole chunk and in the emitted
 * action; no other environment changes; the state row of an environment that is not due is not read.  Built for width 64, 4 heads, latent 32, obs_dim <= 32,
 * 1 <= A <= 8, 1 <= T <= 8, 1 .. 4 encoder and 1 .. 8 decoder layers: D3IL_EUNSUPPORTED otherwise, answered before any launch.  Packed arrays 16-byte aligned. */
int d3il_act_chunk_f32(const float* state, const float* w_in, const float* tab, const float* enc_w, const float* enc_v, const float* dec_w, const float* dec_v,
                       const float* head_w, const float* lo, const float* hi, const float* scale, const float* shift, uint64_t seed, uint64_t env_offset,
                       const uint32_t* t_device, const float* latent_in, int32_t* counter, float* chunk, float* actions, float* latent_out, long n_env, int obs_dim, int A,
                       int T, int width, int n_head, int latent, int n_enc, int n_dec, void* stream);
/* One step of the batched DDPM-ACT policy (policies.DDPMACTPolicy; ddpm_encdec_agent.py:222-257 around diffusion_policy.py:117-217 and diffusion_models.py:844-905,
 * no goals) in one launch, f32 throughout.  Persistent per-environment state on the device: counter i32 [n_env] and chunk [n_env][action_seq_len][A] (already clamped
 * and inverse-scaled).  An environment with counter == action_seq_len (or outside 0 .. action_seq_len) is due and runs the whole reverse chain on its window
 * (window [n_env][obs_seq_len][obs_dim], scaled, left-aligned, oldest first; len i64 [n_env] valid rows, 1 .. obs_seq_len): x = normals of chain index T =
 * n_timesteps; for i = T - 1 .. 0: encoder on [temb[i], (W_tok s + b_tok) + pos[0 .. L-1]] (causal; LayerNorm with weight only, eps 1e-5; exact GELU), decoder on the
 * action tokens (W_act x_t + b_act) + pos[L - 1 + t] (causal self-attention plus unmasked cross-attention over the 1 + L encoder rows in front of one projection),
 * eps = head; x0 = clamp(sched[i][0] x - sched[i][1] eps, lo, hi), x = sched[i][2] x0 + sched[i][3] x + sched[i][4] normals_i (i = 0: nothing drawn or added); then
 * chunk[n][t][a] = clamp(x, lo_a, hi_a) scale_a + shift_a and counter = 0.  Every environment then emits actions[n] = chunk[n][counter] and stores counter + 1.  A
 * workgroup (16 environments) without a due environment runs no network; an environment's result never depends on which of its neighbours are due or on their
 * window lengths.  Random numbers: Philox4x32-10, key = seed, counter = (env_offset + n, *t_device, 0x44410000 | k << 8 | t << 1 | q), k the chain index, t the action
 * token, component 4 q + m, normals as d3il_ddpm_gpt_step_f32.  w_in, tab, enc_w, enc_v, dec_w, dec_v, head_w: policies.pack_ddpm_act_weights (fragment order as
 * d3il_act_chunk_f32; w_in = tok_emb (32 columns) | action_emb (16 columns); layer arrays as d3il_act_chunk_f32; tab = pos [8][64] | encoder ln | decoder ln |
 * tok_emb bias | action_emb bias | head bias [16] | temb [T][64] | sched [T][5]); lo / hi (scaled space) / scale / shift [A]; t_device: DEVICE u32, read only.
 * Optional (NULL): noise_in [n_env][T + 1][action_seq_len][A] replaces the draws (index = chain index); x_in [n_env][action_seq_len][A] replaces the first
 * iterate; k_start < 0 runs the whole chain, otherwise only chain steps k_start .. k_stop (0 <= k_stop <= k_start + 1 <= T; k_stop = k_start + 1: no step, the
 * first iterate goes to the final clamp) - test hooks; x_out [n_env][action_seq_len][A] the iterate after the last step run (before the final clamp), noise_out
 * (layout of noise_in) what was drawn - both written for due environments only; bad i32 [n_env] (may be NULL): 1 for a due
 * environment with a NaN / Inf in a valid window row, a head output or an iterate - it gets NaN in its whole chunk and in the emitted action -, 0 for every other
 * one.  No other environment changes; padding rows and the window of an environment that is not due are not read.  Built for width 64, 4 heads, obs_dim 1 .. 32,
 * 1 <= A <= 8, obs_seq_len 1 .. 5, action_seq_len 1 .. 4, 1 .. 4 encoder and 1 .. 8 decoder layers, 1 .. 255 timesteps, linear_head = 1: D3IL_EUNSUPPORTED
 * otherwise, answered before any launch.  Packed arrays 16-byte aligned. */
int d3il_ddpm_act_chunk_f32(const float* window, const int64_t* len, const float* w_in, const float* tab, const float* enc_w, const float* enc_v, const float* dec_w,
                            const float* dec_v, const float* head_w, const float* lo, const float* hi, const float* scale, const float* shift, uint64_t seed,
                            uint64_t env_offset, const uint32_t* t_device, const float* noise_in, const float* x_in, int32_t* counter, float* chunk, float* actions,
                            int32_t* bad, float* x_out, float* noise_out, long n_env, int obs_dim, int A, int obs_seq_len, int action_seq_len, int width, int n_head,
                            int n_enc, int n_dec, int n_timesteps, int linear_head, int k_start, int k_stop, void* stream);
/* The whole inference of the batched conditional-VAE policy (policies.CVAEPolicy; cvae_agent.py:155-170 around cvae.py:55-62) in one launch, f32 throughout: per
 * environment z = clamp(z_in[n] or `latent` Box-Muller normals, -0.5, 0.5) (the reference clamps its prior sample: 61.7 % of the components sit on a bound), the
 * decoder (ResidualMLPNetwork, Mish) on the row [state | z], actions[n][a] = clamp(out_a, lo_a, hi_a) scale_a + shift_a (product and sum in f64, rounded once).
 * Random numbers: Philox4x32-10, key = seed, counter = (env_offset + n, *t_device, 0x43560000 | q), q < 8; component 4 q + m from word m, normals as
 * d3il_ddpm_gpt_step_f32.  state [n_env][obs_dim] (scaled); w_in: the input layer packed to 64 columns, [NT][64][16] (policies.pack_resmlp_weights with
 * in_cols=64; NT = hidden / 16); b_in .. b_out as d3il_resmlp_f32; lo / hi (scaled space) / scale / shift [A]; t_device: DEVICE u32, read only.  z_in [n_env][latent]
 * (unclamped) and z_out [n_env][latent] (the clamped latent that was used) may be NULL.  An environment with a NaN / Inf in its state row, in its unclamped latent
 * or in a decoder output gets NaN in every action component (z_out: NaN where the latent was hit); no other environment changes.  Built for hidden 128 / 256,
 * 1 <= latent <= 32, obs_dim >= 1, obs_dim + latent <= 64, 1 <= A <= 16, n_blocks >= 0: D3IL_EUNSUPPORTED otherwise, answered before any launch.  Packed arrays
 * 16-byte aligned. */
int d3il_cvae_decode_f32(const float* state, const float* w_in, const float* b_in, const float* w_blocks, const float* b_blocks, const float* w_out, const float* b_out,
                         const float* lo, const float* hi, const float* scale, const float* shift, uint64_t seed, uint64_t env_offset, const uint32_t* t_device,
                         const float* z_in, float* actions, float* z_out, long n_env, int obs_dim, int latent, int A, int hidden, int n_blocks, void* stream);
/* The whole reverse chain of the batched DDPM-MLP policy (policies.DDPMNativePolicy; ddpm_agent.py:213-274 around gc_diffusion.py:101-216 over
 * diffusion_models.py:20-118) in one launch, f32 throughout, on the Philox stream: per environment x = z_0; for i = n_timesteps - 1 .. 0: eps =
 * ResidualMLPNetwork([x | temb[i] | state]) (Mish), x0 = clamp(sched[i][0] x - sched[i][1] eps, lo, hi), x = (sched[i][2] x0 + sched[i][3] x) + sched[i][4] z_k with
 * k = 1 + (n_timesteps - 1 - i) (i = 0: nothing drawn or added); actions[n][a] = clamp(x_a, lo_a, hi_a) scale_a + shift_a (product and sum in f32).
 * z_k = noise_in[k][n][a] when given, otherwise Box-Muller normals as d3il_ddpm_gpt_step_f32 on Philox4x32-10 with key = seed and counter = (env_offset + n,
 * *t_device, 0x444D0000 | k << 1 | q), component a = 4 q + m; n_timesteps draws per call, k = 0 .. n_timesteps - 1.  t_device: DEVICE u32, read only.  state
 * [n_env][obs_dim] (scaled).  The input layer comes split by column group (policies.pack_ddpm_mlp_weights): w_x [NT][64][2] the A columns of x packed to 8
 * ([T_out][lane (g, i)][s] = W[16 T_out + i][4 s + g]; NT = hidden / 16), w_state [NT][64][16] the obs_dim state columns packed to 64 in the same order, tbias
 * [n_timesteps][hidden] = W[:, A .. A + t_dim - 1] temb[i] + b_in; w_blocks .. b_out as d3il_resmlp_f32; sched [n_timesteps][5] (policies.ddpm_schedule);
 * lo / hi (scaled space) / scale / shift [A].  noise_in [n_timesteps][n_env][A] may be NULL; noise_out [n_timesteps + 1][n_env][A] (what was used; the last entry,
 * the step i = 0, is zeros) may be NULL.  bad i32 [n_env]: 1 for an environment with a NaN / Inf in its state row, in a draw it uses, in an eps or in its final x -
 * it gets NaN in every action component -, 0 otherwise; no other environment changes.  Built for hidden 128 / 256, 1 <= A <= 8, obs_dim >= 1, A + t_dim + obs_dim
 * <= 64 input columns, 1 <= n_timesteps <= 255, n_blocks >= 0: D3IL_EUNSUPPORTED otherwise (n_timesteps < 1: D3IL_EINVAL), answered before any launch.  Packed
 * arrays 16-byte aligned.  (No _f32 suffix and the step word first: capi.SIGNATURES3 holds this entry.) */
int d3il_ddpm_mlp_chain(const uint32_t* t_device, const float* state, const float* w_x, const float* w_state, const float* tbias, const float* w_blocks,
                        const float* b_blocks, const float* w_out, const float* b_out, const float* sched, const float* lo, const float* hi, const float* scale,
                        const float* shift, uint64_t seed, uint64_t env_offset, const float* noise_in, float* actions, int32_t* bad, float* noise_out, long n_env,
                        int obs_dim, int A, int t_dim, int n_timesteps, int hidden, int n_blocks, void* stream);
/* The whole inference of the batched BeT-MLP policy (policies.BeTMLPPolicy; bet_mlp_agent.py:366-406 around generate_latents, 114-147, and k_means.py
 * decode_actions) in one launch, f32: per environment h = the input layer and the residual blocks of the ResidualMLPNetwork (Mish) on the scaled state row,
 * logit_v = w_out[v] . h + b_out[v] for v < 64, p = exp(logit - max) with inclusive prefix sums c and S = c_63, u = u_in[n] or 24 bits of Philox4x32-10 (key = seed,
 * counter = (env_offset + n, *t_device, 0x424D4C50)), bins[n] = min(#{v : c_v <= u S}, 63), off_a = w_out[64 + bin A + a] . h + b_out[64 + bin A + a] (layout
 * "(V A)"), actions[n][a] = clamp(centers[bin][a] + off_a, lo_a, hi_a) scale_a + shift_a (sum and clamp in f32; product and sum in f64, rounded once).
 * state [n_env][obs_dim] (scaled); w_in, b_in, w_blocks, b_blocks as d3il_resmlp_f32 (input layer packed to 32 columns); w_logit: rows 0 .. 63 of the output layer
 * packed like d3il_resmlp_f32's w_out tiles, [4][NT][64][4] (NT = hidden / 16; policies.pack_bet_mlp_weights), b_logit [64]; w_off: rows 64 .. of the output layer
 * row-major [64 A][hidden], b_off [64 A]; centers [64][A]; lo / hi (scaled space) / scale / shift [A]; t_device: DEVICE u32, read only.  u_in [n_env], u_out [n_env]
 * (the uniform that was used) and probs [n_env][64] (p / S) may be NULL.  An environment with a NaN / Inf in its state row, in its final hidden row or in a logit
 * gets bins = -1 and NaN in every action component; no other environment changes.  Built for hidden 128 / 256, V = 64, 1 <= obs_dim <= 28, 1 <= A <= 8,
 * n_blocks >= 0: D3IL_EUNSUPPORTED otherwise, answered before any launch.  Packed arrays, biases and w_off 16-byte aligned. */
int d3il_bet_mlp_f32(const float* state, const float* w_in, const float* b_in, const float* w_blocks, const float* b_blocks, const float* w_logit, const float* b_logit,
                     const float* w_off, const float* b_off, const float* centers, const float* lo, const float* hi, const float* scale, const float* shift, uint64_t seed,
                     uint64_t env_offset, const uint32_t* t_device, const float* u_in, float* actions, int32_t* bins, float* u_out, float* probs, long n_env, int obs_dim,
                     int V, int A, int hidden, int n_blocks, void* stream);
/* The whole inference of the batched BC-GMM policy (policies.BCGMMPolicy; agents/models/gmm/bc_gmm.py:13-90 sampled once per step) in one launch, f32, on the Philox
 * stream: per environment h = the input layer and the residual blocks of the ResidualMLPNetwork (Mish) on the scaled state row, f = Mish(w_feat h + b_feat) (the
 * network's own output layer, hidden rows), logit_g = w_logit[g] . f + b_logit[g] for g < G, p = exp(logit - max) with inclusive prefix sums c and S = c_{G-1},
 * u = u_in[n] or 24 bits of word 0 of Philox4x32-10 (key = seed, counter = (env_offset + n, *t_device, 0x474D0000)), comps[n] = k = min(#{g < G : c_g <= u S}, G - 1),
 * mean_a = 0.01 tanh(w_mean[k A + a] . f + b_mean[k A + a]) (layout "(G A)"), std_a = 1e-4 (std_mode 0: w_std / b_std are never read and may be NULL) or
 * act(w_std[k A + a] . f + b_std[k A + a]) + min_std with act = exp (std_mode 1) or softplus with the switch to the identity above 20 (std_mode 2), z_a =
 * z_in[n][a] or Box-Muller normals as d3il_cvae_decode_f32 on the counter word 0x474D0000 | q, q = 1 + a / 4, component a = 4 (q - 1) + m from word m,
 * actions[n][a] = clamp(mean_a + std_a z_a, lo_a, hi_a) scale_a + shift_a (f32 up to the clamp; product and sum in f64, rounded once).  t_device: DEVICE u32, read
 * only.  state [n_env][obs_dim] (scaled); w_in, b_in, w_blocks, b_blocks as d3il_resmlp_f32 (input layer packed to 32 columns); w_feat [NT][NT][64][4] packed like a
 * block layer (NT = hidden / 16), b_feat [hidden]; w_logit: the G logit rows padded to 64 with zeros and packed like d3il_bet_mlp_f32's, [4][NT][64][4], b_logit [64]
 * (policies.pack_bc_gmm_weights); w_mean / w_std row-major [G A][hidden], b_mean / b_std [G A]; lo / hi (scaled space) / scale / shift [A].  u_in [n_env], z_in
 * [n_env][A], u_out [n_env], z_out [n_env][A] (what was used) and probs [n_env][G] (p / S) may be NULL.  An environment with a NaN / Inf in its state row, in f, in a
 * logit g < G, in a selected raw mean or std, in its std (an overflowing exp) or in a normal it uses gets comps = -1 and NaN in every action component; no other
 * environment changes.  Built for hidden 128 / 256, 1 <= obs_dim <= 28, 1 <= G <= 64, 1 <= A <= 8, n_blocks >= 0, std_mode 0 / 1 / 2: D3IL_EUNSUPPORTED otherwise,
 * answered before any launch.  Packed arrays, b_in .. b_logit, w_mean and w_std 16-byte aligned.  (No _f32 suffix and the row count first: capi.SIGNATURES4 holds this
 * entry.) */
int d3il_bc_gmm(long n_env, const uint32_t* t_device, const float* state, const float* w_in, const float* b_in, const float* w_blocks, const float* b_blocks,
                const float* w_feat, const float* b_feat, const float* w_logit, const float* b_logit, const float* w_mean, const float* b_mean, const float* w_std,
                const float* b_std, const float* lo, const float* hi, const float* scale, const float* shift, uint64_t seed, uint64_t env_offset, const float* u_in,
                const float* z_in, float* actions, int32_t* comps, float* u_out, float* z_out, float* probs, int obs_dim, int G, int A, int hidden, int n_blocks,
                int std_mode, float min_std, void* stream);
/* The tail of the batched BC-GPT policy (policies.GPTBCPolicy; gpt_bc_agent.py:221-247 around gpt_policy.py MinGPT) in one launch: per row x = LayerNorm(h)
 * (biased variance), o_a = w_head[a] . x (no bias), actions[row][a] = clamp(o_a, lo_a, hi_a) scale_a + shift_a (clamp in f32; product and sum in f64, rounded once).
 * h [rows][C] (the last block's output at every environment's last token, before ln_f); ln_weight / ln_bias [C]; w_head [A][C] row-major; lo / hi (scaled space) /
 * scale / shift [A]; bad i32 [rows] (may be NULL): 1 for a row with a NaN / Inf in h, in the normalised row or in a head output - it gets NaN in every action
 * component -, 0 for every other one.  No other row changes.  No random numbers.  Built for C <= 128 (a multiple of 4) and 1 <= A <= 16: D3IL_EUNSUPPORTED otherwise,
 * answered before any launch. */
int d3il_gpt_bc_head_f32(const float* h, const float* ln_weight, const float* ln_bias, float ln_eps, const float* w_head, const float* lo, const float* hi, const float* scale,
                         const float* shift, float* actions, int32_t* bad, long rows, int C, int A, void* stream);
/* Range / NaN guard of the three split-f16 entry points above (opt-in; off = the kernels and results of a library without it).
 * counts_device: device i64[4] owned and zeroed by the caller, or NULL = guard off (the default).  Process-wide: ONE pointer, to the memory of ONE device - for a
 * process that drives one GPU (as every process of this project does); it is not synchronised - set it while no other thread launches these kernels.  Read at launch time by d3il_linear120_f16x3,
 * d3il_mlp_ln_gelu_residual_f16x3, d3il_attn_half_f16x3 and d3il_gpt_trunk72_f16x3, which then launch the guarded instantiation of their kernel.  The call itself touches no device.
 * Split sites: the input row after its LayerNorm (all three), the row's 480 GELU outputs (MLP), the row's 120 attention outputs (attention half).  At a site
 *   a finite operand with |x| > 65504 saturates exactly as without the guard - the row's output is bit-identical - and the row is marked clipped;
 *   a NaN / +-Inf operand goes to the matrix core as NaN: the row is NaN in every output column (as from the f32 entry points), no other row changes, and the row
 *   is marked non-finite.
 * Every launch adds to counts[D3IL_HXG_CLIPPED] / [D3IL_HXG_NONFINITE] the number of its rows (rows < `rows`; tokens < T of sequences < n_seq) with that mark - a row
 * at most once per counter and launch, possibly in both - and 1 to counts[D3IL_HXG_LAUNCHES]; counts[3] is reserved and not touched.  The same row is counted again by
 * every later launch it passes through non-finite (a NaN token travels down the blocks), so the counters tell WHETHER and roughly where, not how many operands.
 * A captured graph keeps the pointer (and the instantiation) it was captured with: capture again after changing the guard.  The packed WEIGHTS are split on the
 * host (policies.split_f16, saturating too); policies.BESOPolicy.range_report counts their out-of-range entries. */
enum { D3IL_HXG_CLIPPED = 0, D3IL_HXG_NONFINITE = 1, D3IL_HXG_LAUNCHES = 2, D3IL_HXG_N = 4 };
int d3il_f16x3_set_guard(long long* counts_device);

/* The whole sampling chain of the reference's DDPM policy in one launch (agents/models/diffusion/gc_diffusion.py:101-216: epsilon prediction, clipped x0, posterior
 * mean, n_timesteps ancestral steps, final clamp; the denoiser = DiffusionMLPNetwork, diffusion_models.py:20-118 over ResidualMLPNetwork, common/mlp.py:114-182: Linear,
 * n_blocks pre-activation residual blocks with Mish, Linear; window 1), f32 on the matrix cores; rows are independent.  All device pointers, f32:
 *   state [rows][state_dim] (scaled observation), noise [n_timesteps + 1][rows][2] (draw 0 = x_T, draw 1 + k = the k-th step's noise), temb [n_timesteps][8] (the time
 *   embedding of step i, row i), sched [n_timesteps][5] = sqrt(1 / acp), sqrt(1 / acp - 1), posterior mean coefficients 1 and 2, sigma (0 for step 0), bounds = min[2] max[2],
 *   out [rows][2] (scaled action); weights in the kernel's tile order (d3il_amd/policies.py pack_ddpm_weights): w_in [16][64][8], w_blocks [2 n_blocks][16][16][64][4],
 *   w_out [16][64][4]; b_in [256], b_blocks [2 n_blocks][256], b_out [2].  Built for hidden 256, action 2, t_dim 8, state_dim <= 18 (D3IL_EUNSUPPORTED otherwise).
 * A row with a NaN / Inf in its state, in one of its n_timesteps + 1 noise draws or in its final x gets NaN (0x7FC00000) in both output components - the clips
 * alone would return a bound, a finite in-bounds action; no other row changes, and finite rows are bit for bit what they are without the test. */
int d3il_ddpm_mlp_f32(const float* state, const float* noise, const float* temb, const float* w_in, const float* b_in, const float* w_blocks, const float* b_blocks,
                      const float* w_out, const float* b_out, const float* sched, const float* bounds, float* out, long rows, int state_dim, int n_timesteps, int hidden,
                      int n_blocks, void* stream);

/* out[rows][out_dim] = the reference's ResidualMLPNetwork (agents/models/common/mlp.py:114-182: Linear, n_blocks pre-activation residual blocks with Mish, Linear; the
 * network of BC_Agent.predict, bc_agent.py:240-271) of x [rows][in_dim] in one launch on the f32 matrix cores.  Weights in the kernel's tile order
 * (d3il_amd/policies.py pack_resmlp_weights; NT = hidden / 16): w_in [NT][64][8], w_blocks [2 n_blocks][NT][NT][64][4], w_out [NT][64][4]; b_in [hidden],
 * b_blocks [2 n_blocks][hidden], b_out [16] (padded).  Built for hidden 128 / 256, in_dim <= 28, out_dim <= 16 (D3IL_EUNSUPPORTED otherwise).
 * Nothing clips here, so a NaN / Inf in a row of x travels through the products by itself: that row comes out NaN in every column (an Inf meets weights of both
 * signs in the first sum over a hidden layer), no other row changes - rows are independent, dead tail lanes re-read the last row and store nothing. */
int d3il_resmlp_f32(const float* x, const float* w_in, const float* b_in, const float* w_blocks, const float* b_blocks, const float* w_out, const float* b_out, float* out, long rows,
                    int in_dim, int hidden, int n_blocks, int out_dim, void* stream);

/* Per-context episode tally, filled by d3il_auto_reset before it resets: table i64 [n_ctx][D3IL_TALLY_ROW] (caller-owned device
 * memory, caller zeroes it), row ctx_id[env] (device i32[n_envs]; NULL = row 0) += {episodes, successes, successes by mode code}
 * with the mode code = Avoiding: 9-bit mode encoding; Pushing: info['mode'] + 1; Sorting: np.packbits code.  These are the
 * integer tables the metric tails work from (avoiding_sim.py:128-135, pushing_sim.py:140-167, sorting_sim.py:191-208) and the
 * input of the single cross-GPU all-reduce.  table = NULL switches the tally off.
 * Stacking: order code of D3IL_SFLAG_MODE_MASK (< 256) and, because info['success_1'] / ['success_2'] (stacking_sim.py:118-136) also count
 * episodes that did not stack all three boxes, row[2 + D3IL_TALLY_ALL + code] += 1 for EVERY finished episode. */
enum { D3IL_TALLY_ROW = 2 + 512, D3IL_TALLY_ALL = 256 };
int d3il_set_tally(d3il_handle h, const int32_t* ctx_id_device, int n_ctx, int64_t* table_device);

/* Integer metric counts on device: out_counts i64[2 + 512] = {n_done, n_success, histogram of 9-bit mode codes
 * among successful envs}; input to the cross-GPU reduction (one RCCL all-reduce, done by the Python layer)
 * and to success-rate / entropy (avoiding_sim.py:128-135). */
int d3il_count_metrics(d3il_handle h, int64_t* out_counts_device, void* stream);

/* The one exchange step of the path: the int64 metric tables of all GPUs are summed with ONE RCCL all-reduce over xGMI, issued by
 * the library on the caller's stream.  Replaces the shared-memory tensors the reference's worker processes write their results into
 * (avoiding_sim.py:104-118 `successes` / `mode_encoding` with share_memory_(), pushing_sim.py:96-131, sorting_sim.py:144-181,
 * stacking_sim.py:182-216).  RCCL is resolved at run time (an RCCL already in the process - PyTorch's - or librccl.so), so the library
 * does not link it.  Protocol: rank 0 calls d3il_comm_unique_id and hands the 128 bytes to the other ranks by any host channel (bench.py:
 * a torch.distributed broadcast); every rank calls d3il_comm_init(id, rank, world, device_id) - collective -, then
 * d3il_reduce_metrics(h, comm, table, count, stream) in place on device i64[count] (table = NULL: the table of d3il_set_tally), and
 * d3il_comm_destroy.  Integer sums: bit-exact, independent of rank order and of the number of GPUs. */
typedef struct d3il_comm_s* d3il_comm;
typedef struct { char internal[128]; } d3il_rccl_unique_id;   /* = ncclUniqueId */
int d3il_rccl_available(void);                         /* 1 when RCCL could be resolved in this process (no communicator is made) */
int d3il_comm_unique_id(d3il_rccl_unique_id* out);
int d3il_comm_init(const d3il_rccl_unique_id* id, int rank, int world, int device_id, d3il_comm* out);
int d3il_comm_count(d3il_comm comm, int* ranks);       /* ncclCommCount: the number of ranks RCCL itself sees in this communicator */
int d3il_comm_destroy(d3il_comm comm);
int d3il_reduce_metrics(d3il_handle h, d3il_comm comm, int64_t* table_device, size_t count, void* stream);

/* Timing of the last d3il_step kernel launch on its own stream (HIP events recorded around the launch when
 * enabled); used by bench.py for the roofline figure. */
int d3il_set_timing(d3il_handle h, int enabled);
int d3il_last_step_ms(d3il_handle h, float* ms);
/* With timing enabled EVERY d3il_step launch gets its own event pair (a ring of 128; a pair is read when its slot comes round again, so the host never waits
 * for a launch it has just enqueued).  Drains the ring and returns out4 = {sum of the launch durations in ms, min, max, number of launches} since d3il_set_timing(h, 1). */
int d3il_timing_stats(d3il_handle h, double* out4);
/* One host call for one iteration of the rollout loops (fewer trips through the binding when a GPU's environments are stepped as several sub-batches):
 * d3il_step_auto_reset = d3il_step + d3il_auto_reset; d3il_random_rollout_step = d3il_policy_action + d3il_step + d3il_auto_reset (BASELINE config 2).
 * d3il_random_rollout_step with option "fuse_rollout_tail" (Avoiding): a call that continues the previous one (same seed, env_offset, actions, stream, t = previous
 * t + 1, nothing else called on the handle in between) is ONE kernel launch - the split step kernel, whose physics wave does for its own environment, after
 * the step, what the harness does between two steps: last_reset mask, episode counters and tally, reset of a finished environment from the handle's cached
 * post-reset image (d3il_start computes it once per init_qpos with the reset kernel itself), re-latch of the harness pose, and the policy's action for step t + 1,
 * which it leaves in `actions`.  The first call of a sequence launches the policy kernel first.  Any other call that reads or writes the harness pose or the actions
 * (d3il_reset, d3il_step, d3il_set_state, d3il_policy_begin / _action, d3il_auto_reset, an option) ends the sequence: the pose is put back to where the prepared
 * draw started.  With the one-wave step kernel (split_waves = 0, lanes_per_wave < 64) the same work runs as a second launch (k_avoiding_tail).
 * Cost of a change: the kernel reads seed, env_offset, `actions` and `episode_counts_device` from a small per-handle device block.  A call in which one of
 * them differs from the previous call rewrites the block and waits for the stream (for the whole device when the stream changed as well) before it launches:
 * once per sequence in a rollout loop, but a host synchronisation per step for a caller that alternates seed or buffers from step to step.
 * Avoiding, split step kernels: in both calls an environment that is finished and not successful when the step begins takes no rare constraint solve (rod
 * contact, arm joint limits) during the step - the reset inside the same call overwrites all it would compute.  What the caller can read afterwards is bit for
 * bit what d3il_step followed by d3il_auto_reset leaves. */
int d3il_step_auto_reset(d3il_handle h, const double* actions, int64_t* episode_counts_device, void* stream);
int d3il_random_rollout_step(d3il_handle h, uint64_t seed, uint64_t env_offset, uint32_t t, double* actions, int64_t* episode_counts_device, void* stream);
/* Step group (Avoiding): up to 8 handles of one device whose d3il_random_rollout_step calls of one step go out as ONE dispatch of
 * sum(ceil(n_i / 64)) workgroups on the first member's stream - for processes whose streams outnumber their hardware queues (GPU_MAX_HW_QUEUES; HIP's default
 * is 4, one of which serves the null stream), where the launches of two sub-batches would share a queue and run one after the other.
 * A call on a member is ELIGIBLE when it would be the one-launch form on its own: option "fuse_rollout_tail", the split step kernel, d3il_start done, no
 * "graph_rollout", and it continues the member's sequence (see above).  An eligible call only marks the member pending and returns; the call that makes every
 * member pending - a ROUND: the same t, n_substeps, max_steps and timing setting for all - launches once.  Results are bit for bit those of the separate launches.
 * CONTRACT: between the first and the last call of a round the buffers of the pending members are NOT yet advanced, and nothing has been enqueued for them;
 * d3il_group_flush ends a round early.  Every call that is not eligible (the first call of a sequence, a jump of t, a member called twice, other arguments) and every
 * other library call on a member that reads or changes its state, buffers, options, timing or tally (d3il_step, d3il_get_state, d3il_reset, d3il_set_option, ...) first
 * flushes the round - each pending member runs through the single-handle path, in group order - and then runs as it does without a group; a round that is never
 * completed is exactly the code path of ungrouped handles.  Two calls that take a handle do NOT end a round: d3il_get_buffers, which only hands out the
 * pointers (what the caller reads through them falls under the contract above), and d3il_set_link_guard, which refuses Avoiding handles.
 * Stream order as seen by the caller is kept: before the merged launch the first member's stream waits for an event recorded on every other member's stream, after it
 * every other member's stream waits for the launch.  Work queued on a member's stream before that member's own call of the round, or after the round's last call,
 * sees what it would see ungrouped.  Work queued on it BETWEEN those two calls is ordered before the step (the event is recorded at the launch), where ungrouped it
 * would come behind it: that is the contract above seen from the stream.
 * Timing: every member counts the merged launch as its launch of that step, with the duration of the whole dispatch (one event pair, shared, owned by the group).
 * A handle that leaves its group reads the durations it still owes from those pairs first, so d3il_timing_stats loses nothing; d3il_last_step_ms of a handle whose
 * last timed launch was a merged one returns D3IL_ESTATE after it left, until its next timed launch.
 * Errors: when a HIP call fails inside a flush or a merged launch, the call that triggered it returns the error and the round is abandoned - deferred steps of
 * members whose calls had already returned D3IL_OK may not have been enqueued, and a member handled before the failure has had its prepared action consumed
 * without a launch.  The sequences of all members are then undefined: reset them (d3il_reset) before stepping on.
 * The third wave runs while the dispatch has at most the sum of the members' "serve_wave_max_workgroups" workgroups.  d3il_destroy of a member flushes and leaves
 * the group; d3il_group_destroy flushes and returns the handles to the single path.  One host thread per group.
 *
 * Group option "quiet_streams" (d3il_group_set_option; default 0 = everything above holds for every round).  With 1 the caller DECLARES:
 * between two merged rounds it queues nothing on the members' streams that reads or writes memory the step touches - the members' buffers, `actions`, the
 * episode counters, the tally - except on the FIRST member's stream, which stays fully ordered.  The library then keeps the post-launch waits (after every
 * round every other member's stream waits for the launch: work queued on a member's stream after a round sees that round, as above) but queues the
 * pre-launch joins - the event on every other member's stream and the first member's wait for it - only in an ARMED round.  A round is armed when it is the
 * first merged round of the group, or the first after any of: a flush of a round (a call that is not eligible or does not fit, d3il_group_flush), any library
 * call on a member other than a merged d3il_random_rollout_step (pending round or not), a member leaving, another stream or `actions` buffer of a member,
 * a switch of this option, a HIP failure.  Every other round CONTINUES the previous one: nothing is recorded or waited for before the launch, the dispatch
 * follows the previous one on the first member's stream.  d3il_group_flush is the caller's re-arming point: it arms the next merged round also when no
 * round is pending.  THE HAZARD, in both directions: a write queued on another member's stream before a continuing round is NOT ordered before that step;
 * and a read queued there after round N is ordered behind round N but NOT before round N+1, which may overwrite what it reads.  In both cases call d3il_group_flush
 * after queueing that work and before the next round (the armed round joins what the streams hold when it launches), or use the first member's stream.
 * d3il_group_stats: merged rounds and merged rounds that joined, since the group was created; plain host counters (no flush, no device access).  With the
 * option off the two are equal.
 *
 * Group option "dispatch_sets" (d3il_group_set_option; default 1 = everything above holds as written).  With K the members, in the order given
 * to d3il_group_create, form K contiguous runs of as equal a member count as possible (the first count % K runs hold one more): DISPATCH SETS.  K below 1 or above
 * the number of live members is D3IL_EINVAL; setting the option flushes and arms, like "quiet_streams", and a handle that moves to another set answers
 * d3il_last_step_ms as one that left a group (above).  A set launches on its own: when all ITS members are pending, as one dispatch of the set's workgroups on
 * the stream of its first live member (the set's LEADER), without waiting for the other sets.  Read everything above with "the set" for "the group" and "the
 * leader" for "the first member": a round and its key (t, n_substeps, max_steps, timing) are those of one set, so set A may be several steps ahead of set B;
 * the pre-launch joins, "quiet_streams" with its armed flag, and the post-launch waits concern the set's other members' streams only; the third wave runs while
 * the set's workgroups stay within the sum of ITS members' "serve_wave_max_workgroups"; the timing pair is the set's, entered into its members' rings (the
 * members of one set report the same durations, members of different sets their own).  Nothing is recorded on, or waited for by, a stream of another set in a
 * running sequence.  No ordering between the sets is needed, because everything a step touches is per handle: the members' buffers, `actions`, the episode
 * counters and the tally belong to one member, hence to one set.  A caller that shares one of them between members of different sets (one tally table, one
 * counter) gets the atomic adds of both dispatches in either order - sums are the same - but must not read them before both sets have run the step it asks for.
 * Under "quiet_streams" the stream that stays fully ordered for a member's buffers is its own set's leader's.
 * Ending a round stays on the side of joining: whatever ends a round above (a call that is not eligible or does not fit ITS set's round, a second call of a
 * pending member, any other library call on a member, d3il_group_flush, a member leaving, a HIP failure) ends the pending rounds of ALL sets and arms all of
 * them.  A member that leaves shrinks its set (the next live member leads it); a set without a live member is skipped; a set of one member still launches the
 * group form.  d3il_group_stats counts merged DISPATCHES, and those that joined: K per step when every set merges.
 *
 * Group option "pipeline_depth" (d3il_group_set_option; default 1 = everything above holds as written).  With D = 2 .. 4 consecutive merged
 * rounds of the group overlap: round r of a running sequence launches on the r mod D-th of the group's LAUNCH STREAMS (the first D distinct member streams, in
 * group order) with no event between the rounds, and on the device every workgroup of round r waits for its own predecessor of round r - 1 - the only
 * workgroup whose stores it reads - so a workgroup no longer waits for the slowest workgroup of the previous dispatch.  Results are bit for bit those of depth 1.
 * D >= 2 needs "quiet_streams" 1 and "dispatch_sets" 1 (D3IL_EINVAL otherwise, also when one of those two is changed while D >= 2).  A round is pipelined
 * only while a waiting workgroup can never keep its predecessor off the chip: the three-wave form (one workgroup per CU) and D x (workgroups of the dispatch) <=
 * the device's CU count (group option "pipeline_cu_budget", 1 .. the device's count, lowers what is counted on - for a process that shares the chip with
 * other resident work); a group that does not meet this, or whose members share streams so that fewer than two launch streams exist, silently runs with depth 1.
 * CONTRACT of a pipelined sequence, on top of "quiet_streams": between two rounds NO member stream - the first member's included - is ordered with respect to
 * the memory the step touches; rounds are in flight on several of them.  Whatever arms a round under "quiet_streams" (above: d3il_group_flush, any other
 * library call on a member, a call that is not eligible, a member leaving, an option switch, a HIP failure) also ENDS the sequence: every member stream then
 * waits for the last round of every launch stream, so work queued on a member's stream after that point sees every round, and the next merged round starts a
 * new sequence behind what the member streams hold (the join of an armed round, then the epoch words are zeroed and the other launch streams let go).  A
 * device or stream synchronisation by the caller orders the host as usual.  So: read or write the step's memory only behind d3il_group_flush (or another
 * library call on a member) or behind a device synchronisation.
 * Timing: the event pair of a pipelined round lies around its launch on its launch stream; the duration includes the time its workgroups waited for their
 * predecessors, so it is no longer the time the step's arithmetic takes.
 * The wait of a workgroup is bounded by the group option "pipeline_timeout_ms" (default 2000, 1 .. 600000).  A workgroup that gives up - the limit ran out, or
 * the group's fault word is already set - sets the fault word, does NOT step, and lets its successors go, which give up at once: a faulted sequence drains in
 * microseconds.  The library reads the fault word wherever it waits for the device on behalf of a member - d3il_get_state, d3il_timing_stats, d3il_destroy of a
 * member, d3il_group_destroy - and answers D3IL_ESTATE once per fault (the word is then cleared): the members do not hold the state after the steps called.
 * d3il_group_pipeline_stats: merged rounds that were pipelined, and faults reported, since the group was created; host counters. */
typedef struct d3il_group_s* d3il_group;
int d3il_group_create(const d3il_handle* handles, int count, d3il_group* out);
int d3il_group_flush(d3il_group g);
int d3il_group_set_option(d3il_group g, const char* name, int value);
int d3il_group_stats(d3il_group g, int64_t* merged_rounds, int64_t* joined_rounds);
int d3il_group_pipeline_stats(d3il_group g, int64_t* pipelined_rounds, int64_t* pipeline_faults);
int d3il_group_destroy(d3il_group g);
/* Option "graph_rollout": captures the graphs the next d3il_random_rollout_step calls with these arguments will launch, without launching anything (outside a timed region). */
int d3il_random_rollout_prepare(d3il_handle h, uint64_t seed, uint64_t env_offset, uint32_t t, double* actions, int64_t* episode_counts_device, void* stream);

/* "ik_fast_path" (default 1), "split_waves" (-1 auto, 0, 1), "lanes_per_wave", "lds_pad_bytes";
 * "serve_wave_max_workgroups" (default 256): Avoiding - up to this many workgroups (64 environments each) the split kernel runs with a third wave that executes the
 * rare constraint paths (rod contact, arm joint limits) for the physics wave; above it (more than one workgroup per CU) the two-wave form runs; 0 = always two waves (A/B);
 * "solver_strict" (default 0): 1 = the contact solvers of Pushing / Sorting / Stacking iterate to round-off like the CPU oracle (parity A/B);
 * "stack_reset_coop" (default 1): Stacking env.reset() through the step kernel's wave-cooperative phases, 0 = the one-lane reset kernel (A/B);
 * "graph_rollout" (default 0): Avoiding - d3il_random_rollout_step is captured once per handle (HIP graph: policy kernel with the step counter in device memory,
 * step kernel, mask copy, tally, auto-reset, counter + 1) and a step becomes ONE hipGraphLaunch instead of eight runtime calls; needs a non-null stream
 * (the legacy default stream cannot be captured); any later option / timing / tally change drops the graphs, the next call re-captures.  With timing enabled every
 * eighth step runs uncaptured with the event pair around its step launch (event nodes inside a graph give no timestamps with this runtime): d3il_timing_stats
 * then covers a uniform 1-in-8 sample of the launches;
 * "fuse_rollout_tail" (default 0): Avoiding - d3il_random_rollout_step as ONE launch: the split step kernel does everything between two steps as its epilogue
 * (last_reset mask, episode counters and tally of the finished environments, their reset and re-latch, and the policy's action for the NEXT step - which the
 * next call of an uninterrupted sequence finds in `actions`); two launches with the one-wave step kernel; same results as the five launches and the copy it
 * replaces. */
int d3il_set_option(d3il_handle h, const char* name, int value);
/* Link-near guard of the generic engine (Pushing / Sorting / Inserting; csrc/link_guard.h).  The engine collides only the rod with the scene; the model's other robot
 * collision hulls (panda_rod_invisible.xml: link0 .. link7, hand, fingers, finger tips) are not evaluated.  With capsules set, every d3il_step ends with one more small
 * kernel on the caller's stream that places the capsules by forward kinematics (qpos rows 0 .. 8) and raises D3IL_PFLAG_LINK_NEAR in the flag word of every environment
 * in which a capsule is closer than `margin` to a cube or - capsules with the second word set - to a static box.  The bit is sticky for the episode and cleared by
 * d3il_reset / d3il_auto_reset like the other per-episode bits; the physics is not touched.  The test samples env-step boundaries: a persisting approach cannot be missed,
 * one shorter than an env step can.  The distance used is a lower bound of the true capsule <-> box distance, at most 1.25e-4 m below it.
 * capsules: HOST f64 [n][9] = body id in the blob's body list (an arm link or a body welded to one, a finger or its tip, link0), 1 = also against the static boxes,
 * p0[3], p1[3] in that body's frame, r.  n = 0 switches the guard off (the default).  flagged_episodes_device (may be NULL): device i64, += 1 whenever an environment's
 * bit goes 0 -> 1, i.e. the number of flagged episodes.  D3IL_EUNSUPPORTED for Avoiding / Stacking / Aligning handles; D3IL_EINVAL for a body outside the chain, r <= 0,
 * margin < 0, n > 16, a segment longer than 1 m.  Synchronises the device; drops captured graphs like any option. */
int d3il_set_link_guard(d3il_handle h, const double* capsules, int n, double margin, int64_t* flagged_episodes_device);
/* Diagnostics builds only (-DD3IL_DEVICE_STATS): per-path lane/wave counters of the step kernel. */
int d3il_debug_stats(uint64_t* out32, int reset);
int d3il_debug_wave_stats(uint64_t* out_nwaves_x10, int nwaves, int reset);
int d3il_debug_wave_counts(uint64_t* out_nwaves_x8, int nwaves, int reset);      /* generic engine: solver event counts per workgroup */
/* Diagnostics: copies `count` doubles of one environment's solver scratch column (contact records of its last physics sub-step)
 * to the host; Pushing / Sorting / Stacking only. */
int d3il_debug_scratch(d3il_handle h, int env, double* out, int count);
/* Diagnostics: what this library was built as, and the layout of the generic engine's record area that d3il_debug_scratch copies.
 * out8[0] = D3IL_BUILD_* bits, [1] doubles per environment (GG_SIZE), [2] records per segment (GEN_SEG; one segment per cube slot, then the arm's),
 * [3] doubles per record (GREC), [4] cube slots (GEN_MAXNB), [5] doubles of an environment's LDS block (GL_SIZE), [6] environments per workgroup, [7] 0. */
enum { D3IL_BUILD_POISON = 1 /* -DD3IL_POISON: the read-before-write guard build of all kernel families */, D3IL_BUILD_SK_POISON = 2 /* the cooperative engine's guard */,
       D3IL_BUILD_STATS = 4 /* -DD3IL_DEVICE_STATS */ };
int d3il_debug_build_flags(int* out8);
const char* d3il_last_error(void);
size_t d3il_blob_sizeof(void);
int d3il_version(void);

#ifdef __cplusplus
}
#endif
#endif
