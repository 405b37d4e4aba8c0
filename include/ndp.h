/* ndp.h -- C ABI of libndp_hip.so: the MI355X (gfx950) implementation of the
 * GAN-training hot path of goodmattg/ndivplanning.
 *
 * The reference has no FFI layer; its boundary for this path is Python
 * (models/gan.py, diversity.py, train_gan.py).  The functions below are what a
 * binding for that path calls (ctypes stub: INTEGRATION.md).  Each one names the
 * reference code it replaces (paths relative to the reference checkout).
 *
 * Conventions (all functions):
 *   - every pointer is a DEVICE pointer to contiguous row-major fp32 unless
 *     stated otherwise; the caller owns every buffer, nothing is allocated or
 *     freed inside, no call synchronises;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); work
 *     is enqueued on it and the call returns immediately (graph-capturable);
 *   - return value 0 = enqueued; non-zero = NDP_E_* and nothing was launched;
 *     ndp_last_error() returns a thread-local message for the last failure;
 *   - no global mutable state: calls from different host threads on different
 *     streams are independent (autograd invokes backward from its own thread).
 *
 * Parameter vectors: the networks' parameters are ONE flat fp32 vector each, in
 * state_dict order fc1.weight, fc1.bias, fc2.weight, ... (weight [out][in]
 * row-major, as nn.Linear stores it).  Gradients and Adam moments use the same
 * layout.  ndp_g_param_count / ndp_d_param_count give the lengths.
 */
#ifndef NDP_H_
#define NDP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NDP_VERSION 136          /* 0.3.2: ndp_fm_* (forward / next-frame model), ndp_fm_backward, ndp_fm_side_stream */

#define NDP_OK            0
#define NDP_E_ARG         1      /* bad argument (shape, alignment, null) */
#define NDP_E_LAUNCH      2      /* hipLaunchKernel / hipMemsetAsync failed */
#define NDP_E_UNSUPPORTED 3      /* valid request this build does not cover */

#define NDP_CODE_DIM      256    /* cat(state_code, target_code): train_gan.py:155 */
#define NDP_ACTION_DIM    4      /* models/gan.py:71,94 */
#define NDP_MAX_NOISE_DIM 16
#define NDP_MAX_SAMPLES   256    /* K, diversity samples per row */
#define NDP_ROW_PAD       32     /* row counts of workspaces are padded to this */

int         ndp_version(void);
const char *ndp_last_error(void);

/* Number of fp32 parameters of Decoder(noise_dim) (models/gan.py:61-71) and of
 * Discriminator() (models/gan.py:89-97): 83,780 at noise_dim 2 and 58,305. */
int64_t ndp_g_param_count(int noise_dim);
int64_t ndp_d_param_count(void);

/* rows rounded up to NDP_ROW_PAD */
int64_t ndp_pad_rows(int64_t rows);

/* ------------------------------------------------------------------ NDiv ---
 * diversity.compute_pairwise_divergence(recodes=x, codes=z), forward and
 * backward in one pass (diversity.py:8-19, 36-41):
 *   loss = sum_{n,i,j} relu(0.8 * dz_ij/sum_j dz_ij - dx_ij/sum_j dx_ij)
 * with the row sums treated as constants in the gradient (diversity.py:18) and
 * a zero sub-gradient where dx_ij == 0 (torch.norm's backward).
 *   x        [n, k, cx]   recodes (generated actions)
 *   z        [n, k, cz]   codes (noise)
 *   loss_out [1]          written (not accumulated)
 *   grad_x   [n, k, cx]   d(grad_scale*loss)/dx, written; may be NULL
 *   partials [ndp_ndiv_partials(n,k)] scratch
 * 1 <= k <= NDP_MAX_SAMPLES, 1 <= cx,cz <= 16.  k == 1 yields NaN like the
 * reference (0/0). */
int64_t ndp_ndiv_partials(int64_t n, int k);
int ndp_ndiv_fwd_bwd(const float *x, int cx, const float *z, int cz, int64_t n, int k,
                     float grad_scale, float *loss_out, float *grad_x, float *partials,
                     void *stream);

/* ---------------------------------------------------------- Generator G ---
 * Decoder.forward (models/gan.py:79-86): action_hat = fc5(relu(fc4(relu(fc3(
 * relu(fc2(relu(fc1(cat[code, noise]))))))))).
 * The input is given as its two parts so that the K-fold repeat of the code
 * (train_gan.py:42-47) never has to be materialised:
 *   code   row r of the network input uses code[(r / code_rep) * ld_code ...+256)
 *   noise  row r uses noise[r * ld_noise ...+noise_dim)
 * For a plain z [m, 256+nz] pass code=z, ld_code=256+nz, code_rep=1,
 * noise=z+256, ld_noise=256+nz.
 *   acts   NULL, or workspace of ndp_g_acts_floats(m) floats receiving the
 *          hidden activations h1..h4 (needed by ndp_g_backward)
 *   action_hat [m, 4] */
int64_t ndp_g_acts_floats(int64_t m);
int ndp_g_forward(const float *g_params, int noise_dim,
                  const float *code, int64_t ld_code, int code_rep,
                  const float *noise, int64_t ld_noise, int64_t m,
                  float *acts, float *action_hat, void *stream);

/* Backward of Decoder.forward for the parameters (what autograd computes at
 * train_gan.py:202 for the Decoder): given d_action [m,4] = dLoss/d action_hat
 * and the activations saved by ndp_g_forward, writes
 *   grad [ndp_g_param_count]  dLoss/d params (written, not accumulated)
 *   ws   scratch of ndp_g_bwd_ws_floats(m, noise_dim) floats
 * No gradient is produced for the network input here (the reference detaches the
 * codes and never differentiates the noise: train_gan.py:152-153, 44); that is
 * ndp_g_input_grad, below. */
int64_t ndp_g_bwd_ws_floats(int64_t m, int noise_dim);
int ndp_g_backward(const float *g_params, int noise_dim,
                   const float *code, int64_t ld_code, int code_rep,
                   const float *noise, int64_t ld_noise, int64_t m,
                   const float *acts, const float *d_action,
                   float *grad, float *ws, void *stream);

/* Gradient with respect to the network input z [m, 256+noise_dim] (row stride ld_z;
 * the plain form of ndp_g_forward's input: code_rep == 1):
 *   d_z [m, 256+noise_dim] (row stride ld_dz) = dY1 . fc1.weight, written.
 * d_action != NULL: the data path of the backward pass runs first (acts: what
 * ndp_g_forward saved) -- no parameter gradient is computed.  d_action == NULL: ws
 * is the workspace an ndp_g_backward call with the same arguments has just filled
 * (one more launch on top of it).  ws: ndp_g_bwd_ws_floats(m, noise_dim) floats. */
int ndp_g_input_grad(const float *g_params, int noise_dim, const float *z, int64_t ld_z,
                     int64_t m, const float *acts, const float *d_action,
                     float *d_z, int64_t ld_dz, float *ws, void *stream);

/* ------------------------------------------------------ Discriminator D ---
 * Discriminator.forward (models/gan.py:104-110): logits = fc4(lrelu(fc3(lrelu(
 * fc2(lrelu(fc1(cat[action, code]))))))), slope 0.01.
 *   action row r uses action[(r / action_rep) * 4 ...+4)
 *   code   row r uses code[(r / code_rep) * ld_code ...+256)
 *   logits [m] */
int ndp_d_forward(const float *d_params,
                  const float *action, int action_rep,
                  const float *code, int64_t ld_code, int code_rep, int64_t m,
                  float *logits, void *stream);

/* Backward of Discriminator.forward given d_logits [m] = dLoss/d logits
 * (recomputes the forward inside the kernel; nothing needs to be saved; the gradient
 * with respect to the code is ndp_d_input_grad's):
 *   grad     [ndp_d_param_count] or NULL   dLoss/d params (written)
 *   d_action [m,4] or NULL                 dLoss/d action (written; needs action_rep==1)
 *   ws       scratch of ndp_d_bwd_ws_floats(m) floats (only used when grad != NULL) */
int64_t ndp_d_bwd_ws_floats(int64_t m);
int ndp_d_backward(const float *d_params,
                   const float *action, int action_rep,
                   const float *code, int64_t ld_code, int code_rep, int64_t m,
                   const float *d_logits, float *grad, float *d_action,
                   float *ws, void *stream);
/* ndp_d_backward that also writes d_code [m,256] (row stride ld_dcode) = dLoss/d code,
 * in the same launch; needs code_rep == 1.  grad and d_action as above (may be NULL). */
int ndp_d_input_grad(const float *d_params,
                     const float *action, int action_rep,
                     const float *code, int64_t ld_code, int code_rep, int64_t m,
                     const float *d_logits, float *grad, float *d_action,
                     float *d_code, int64_t ld_dcode, float *ws, void *stream);

/* ----------------------------------------------------------------- Adam ---
 * torch.optim.Adam.step for one flat parameter vector (train_gan.py:98-104,
 * 184, 203): m += (1-b1)(g-m); v = b2 v + (1-b2) g^2;
 * p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps),  t = step_count[0] + 1.
 * step_count is a DEVICE int32[4] "Adam state word": [0] = number of updates applied
 * so far (the call increments it), [1..3] = scratch owned by the library (the bias
 * corrections of the current update, computed once on the device in fp64), so that a
 * captured graph replays with the right bias correction. */
int ndp_adam_step(float *params, const float *grad, float *exp_avg, float *exp_avg_sq,
                  int64_t n, int32_t *step_count, float lr, float beta1, float beta2,
                  float eps, void *stream);

/* ------------------------------------------------------ fused train step ---
 * One iteration of the train_gan.py loop body (train_gan.py:159-203) on a local
 * shard of `flat` rows (FLAT = batch*(traj_len-1)), each with K = num_sample
 * diversity samples, M = flat*K rows through G and D.  The step is split where
 * a data-parallel driver has to all-reduce gradients; single-GPU training sets
 * fuse_adam = 1 and never sees the gradients.
 *
 *   phase A  ndp_step_d_grads : [first call of the step: G forward]
 *            D(real), D(fake) forward, BCE, D backward  -> D gradient
 *            (train_gan.py:165-183); with fuse_adam the D Adam update too (184).
 *            `actions` / `codes` hold ONE row per FLAT row; the reference feeds D
 *            K = num_sample identical copies of each (repeat_interleave,
 *            train_gan.py:140-156), so on the first call of a step the real pass
 *            runs on the FLAT distinct rows with every row's BCE term and loss
 *            gradient weighted K: the same sums, 1/K of the rows.  Repeat calls
 *            (run_g_forward = 0) run both passes on all M rows.
 *   phase B  ndp_step_g_grads : D(fake) forward with the UPDATED D, G loss,
 *            NDiv loss + gradient, backward through D and G -> G gradient
 *            (train_gan.py:187-202); with fuse_adam the G Adam update too (203)
 *   ndp_adam_step              for the non-fused (data-parallel) case
 *
 * Scaling for data parallelism: BCE terms are means over
 * the GLOBAL row count, so inv_m_global = 1/(M summed over ranks); the NDiv term
 * is a sum and is not scaled.  Gradients of all ranks are then SUMMED.
 */
struct ndp_p2p;
typedef struct ndp_step_config {
  int32_t noise_dim;           /* training.gan.noise_dim  (1..16) */
  int32_t num_sample;          /* training.gan.num_sample (1..256) */
  int64_t flat;                /* local FLAT rows */
  float   inv_m_global;        /* 1 / global M */
  float   pairwise_div_factor; /* training.gan.pairwise_div_factor */
  float   lr, beta1, beta2, eps;
  int32_t fuse_adam;           /* 1: apply Adam inside the phase; 0: leave grads */
  int32_t device_noise;        /* 1: G forward draws the noise itself (see `noise` below) */
  uint64_t noise_seed;         /* stream id of the device noise (e.g. the rank) */
  const struct ndp_p2p *p2p;   /* NULL, or the peer-to-peer gradient exchange (see below): the
                                * kernel that sums the split-K slabs then also SUMS the gradient
                                * over ranks before Adam, so a data-parallel step has the same
                                * launches as a single-GPU step and is graph-capturable */
} ndp_step_config;

/* Caller-owned persistent state of one trainer (all device memory). */
typedef struct ndp_step_buffers {
  float   *g_params, *g_grad, *g_exp_avg, *g_exp_avg_sq;   /* [ndp_g_param_count] */
  float   *d_params, *d_grad, *d_exp_avg, *d_exp_avg_sq;   /* [ndp_d_param_count] */
  int32_t *g_step, *d_step;                                 /* Adam state words, int32[4] each */
  float   *losses;       /* [4]: D_loss, G_loss, pair_div (local shares), unused */
  float   *loss_sums;    /* [4]: running sums of the above (epoch averages) or NULL */
  float   *action_hat;   /* [pad(M), 4] generated actions of the current step */
  float   *workspace;    /* ndp_step_workspace_floats(cfg) floats */
} ndp_step_buffers;

int64_t ndp_step_workspace_floats(const ndp_step_config *cfg);
/* Float offset inside that workspace of what a step leaves behind, for tests.  tensor:
 *   0..3  G's saved activations h1..h4, [pad(M),128] [pad(M),64] [pad(M),128] [pad(M),256] (written by phase A only)
 *   4     factor * dNDiv/d action_hat, [pad(M),4] (written by the NDiv blocks only)
 *   5     dLoss/d action_hat, NDiv term included: what G's backward starts from, [pad(M),4] (phase B)
 *   6..8  D's saved activations h1..h3 of the first D step, [pad(FLAT) + pad(M), 64 | 128 | 256]: the distinct real
 *         rows, then from row pad(FLAT) the fake rows (phase B leaves them alone)
 *   9..11 the same of a repeat D step (run_g_forward = 0), which overwrites 6..8: [2 pad(M), .], real rows then fake rows
 * -1: bad config or index. */
#define NDP_STEP_TENSORS 12
int64_t ndp_step_workspace_offset(const ndp_step_config *cfg, int tensor);
/* For tests, host arithmetic only: the block -> (job, chunk) map of a step's weight-gradient launch
 * (which: 0 = D, 1 = G; first: as run_g_forward), by the function the kernel itself calls.
 * pairs[2 b], pairs[2 b + 1] for block b < min(grid, capacity): the job and row chunk; (-2, -2): an
 * NDiv block.  table[32]: the chunk count of every job of the launch's table (0 past its end; a
 * block whose chunk is not below its job's count returns at once), then in table[28..31] njobs,
 * nwide, wide_chunks, nchunks of the launch.  slab_area[2]: float offset and length of the slabs
 * the launch writes, inside the workspace.  Returns the launch's grid, -1 for a bad argument. */
int64_t ndp_step_wgrad_blocks(const ndp_step_config *cfg, int which, int first, int32_t *pairs,
                              int64_t capacity, int32_t *table, int64_t *slab_area);

/* codes [flat,256], actions [flat,4] (ground truth), noise [flat,K,nz].
 * run_g_forward: 1 on the first D step of an iteration, 0 on repeats
 * (discrim_steps_per_gen > 1 re-uses action_hat, train_gan.py:172).
 * With cfg->device_noise the G forward fills `noise` itself with U[0,1) drawn from the
 * counter-based stream (noise_seed, offset = g_step[0]) -- the torch.FloatTensor(...)
 * .uniform_() of diverse_sampling (train_gan.py:44) without the host round trip -- and
 * the later kernels read it from there; otherwise `noise` is an input. */
int ndp_step_d_grads(const ndp_step_config *cfg, const ndp_step_buffers *buf,
                     const float *codes, const float *actions, float *noise,
                     int run_g_forward, void *stream);
int ndp_step_g_grads(const ndp_step_config *cfg, const ndp_step_buffers *buf,
                     const float *codes, const float *actions, const float *noise,
                     void *stream);

/* The step kernels read the layers' weights from lane-ordered ("packed") copies kept in the
 * workspace; the fused Adam updates refresh them.  Call ndp_step_pack_params once before
 * the first step and again whenever g_params / d_params were written by anything else
 * (checkpoint load, a host-side optimizer, ...). */
int ndp_step_pack_params(const ndp_step_config *cfg, const ndp_step_buffers *buf, void *stream);

/* Non-fused (data-parallel) update: Adam for network `which` (0 = D, 1 = G) from
 * buf->d_grad / buf->g_grad (after the all-reduce), refreshing the packed copies.  Must follow
 * the ndp_step_d_grads / ndp_step_g_grads call that produced the gradient: that call also
 * advanced the network's Adam state word (step count and bias corrections). */
int ndp_step_apply_adam(const ndp_step_config *cfg, const ndp_step_buffers *buf, int which,
                        void *stream);

/* The same device noise stream as a stand-alone call: out[i] = U[0,1) from
 * Philox-4x32-10 keyed by seed, counter (i/4, *offset_dev), word i%4. */
int ndp_uniform_noise(float *out, int64_t n, uint64_t seed, const int32_t *offset_dev,
                      void *stream);

/* ------------------------------------------- peer-to-peer gradient exchange ---
 * The data-parallel exchange of SURVEY.md section 8e (two flat SUM all-reduces
 * per step: 58,305 and 83,780 floats) without a collective library: the
 * reference has no collectives (single process, train_gan.py:115-207); this is
 * what replaces "one optimizer sees the whole batch" when the batch is sharded
 * over one process per GPU.
 *
 * Every rank owns one REGION of device memory (uncached / fine-grained, so that
 * stores arriving over xGMI and the polling loads bypass the caches), exported
 * with hipIpc and mapped by every peer.  One exchange, inside the kernel that
 * has just summed the rank's split-K slabs:
 *   push   each workgroup stores its 256 gradient values into the inbox slot
 *          [src = this rank][step parity] of EVERY peer's region, waits for the
 *          stores to be acknowledged, then sets flag[src][workgroup] = step there
 *          (all accesses are system-scope atomics on uncached memory: no cache
 *          maintenance, no fences);
 *   wait   it polls the flags the peers set in its OWN region (bounded by
 *          timeout_ms: on expiry the region's status word is set, the wait is
 *          skipped from then on and ndp_p2p_status reports it -- never a hang);
 *   sum    own value + the peers' values from its own inbox in rank order
 *          0..world-1: every rank computes bit-identical sums, so the replicas
 *          stay bit-identical, run after run.
 * Inboxes are double-buffered on the step's parity: a peer can be at most one
 * exchange ahead (it needs this rank's next push to go further), so no second
 * barrier is needed.  `step` is the network's Adam step count (state word [0]),
 * which must advance by one per exchange and be the same on all ranks.
 * These are the only functions of the library that allocate or synchronise. */
#define NDP_P2P_MAX_RANKS    8
#define NDP_P2P_HANDLE_BYTES 64          /* sizeof(hipIpcMemHandle_t) */

typedef struct ndp_p2p {
  int32_t world, rank;
  int32_t timeout_ms;                    /* bound of one wait (0 = 10,000) */
  int32_t reserved;
  void   *region[NDP_P2P_MAX_RANKS];     /* region[rank] = own allocation, others = mapped peers */
} ndp_p2p;

int64_t ndp_p2p_region_bytes(void);
int ndp_p2p_region_alloc(void **region);                 /* zero-filled; synchronises */
int ndp_p2p_region_free(void *region);
int ndp_p2p_region_reset(void *region);                  /* zero flags + status; synchronises */
int ndp_p2p_export(void *region, void *handle_out);      /* NDP_P2P_HANDLE_BYTES bytes, host memory */
int ndp_p2p_open(const void *handle, void **mapped_out); /* a PEER process's handle */
int ndp_p2p_close(void *mapped);
/* status word of the own region: 0 = ok, 1 + r = a wait for rank r timed out (HOST int out) */
int ndp_p2p_status(const ndp_p2p *p2p, int32_t *status_out);
/* What the first waiter that gave up was waiting for (HOST int32[NDP_P2P_DIAG_WORDS] out; synchronises):
 * {status code, workgroup, net, expected step, flag value it saw, peer rank, 100 MHz ticks waited, 0}. */
#define NDP_P2P_DIAG_WORDS 8
int ndp_p2p_diagnostics(const ndp_p2p *p2p, int32_t *words_out);
/* Copy the status word to PINNED host memory behind everything already enqueued on `stream`, without
 * synchronising: a training loop polls the value of the previous launch for free and aborts early. */
int ndp_p2p_status_async(const ndp_p2p *p2p, int32_t *pinned_host_out, void *stream);
/* PCI bus id ("0000:c1:00.0") of the CURRENT device into out[len >= 16]: ranks that report the same id
 * share a GPU, and the in-kernel exchange needs every rank's reduce kernel co-resident -- which only a
 * GPU per rank guarantees (ndivplanning_amd/dp.py refuses the exchange for such ranks unless forced). */
int ndp_device_pci_bus_id(char *out, int len);
/* The exchange alone: out[i] = sum over ranks of in[i] (n <= the capacity of `net`'s inbox:
 * ndp_d_param_count() for net 0, ndp_g_param_count(NDP_MAX_NOISE_DIM) for net 1).  step_word:
 * device int32, same value on every rank, larger than at the previous exchange on this net. */
int ndp_p2p_all_reduce(const ndp_p2p *p2p, int net, const float *in, float *out, int64_t n,
                       const int32_t *step_word, void *stream);

/* ------------------------------------------------------------ image encoder ---
 * models.image_autoencoder.Encoder.forward in eval mode without gradient
 * (image_autoencoder.py:35-49; train_gan.py:75-76 loads it, 152-153 calls it under
 * .detach()): images [n,3,128,128] (NCHW, as the reference's loader delivers them) ->
 * codes [n,128].  All six layers are implicit GEMMs on the fp32 matrix pipe (conv1: K = 27
 * padded to one 32-wide step) over NHWC activations kept in `workspace`.
 * packed_params: ndp_encoder_param_floats() floats, BatchNorm (eval: running statistics,
 * eps 1e-5) of conv1..conv3 folded into weights and biases:
 *   conv1  w[27][64] with k = ci*9 + kh*3 + kw, then bias[64];
 *   conv2..conv6  w[Cout][KH][KW][Cin], then bias[Cout]   (in this order, back to back).
 * Images are processed in passes of at most 512; workspace: ndp_encoder_workspace_floats(n). */
int64_t ndp_encoder_param_floats(void);
int64_t ndp_encoder_workspace_floats(int64_t n_images);
int ndp_encoder_forward(const float *packed_params, const float *images, int64_t n_images,
                        float *codes, float *workspace, void *stream);
/* The same from DECODED CAMERA FRAMES: frames_hwc [n][128][128][3] bytes (what PIL's JPEG decoder hands the
 * reference's loader, utils/trajectory_loader.py:48-56).  The reference turns them into its [-1, 1] float tensors on
 * the host -- utils/hdf5_load.py:9-11: (ToTensor()(image) - 0.5) * 2.0, ToTensor = byte -> float32, / 255 -- permutes to
 * CHW and uploads 4 bytes per value (train_gan.py:119-124).  Here the first convolution gathers from the bytes and
 * applies the same three fp32 operations (a 256-entry table): bit-identical codes from a quarter of the upload. */
int ndp_encoder_forward_u8(const float *packed_params, const uint8_t *frames_hwc, int64_t n_images,
                           float *codes, float *workspace, void *stream);

/* ------------------------------------------- forward (next-frame) model ---
 * models.forward_encoder.ForwardAutoencoder (forward_encoder.py:20-114) and one iteration
 * of its training loop (train_forward_model.py:98-112): U-Net of stride-2 convolutions /
 * transposed convolutions with BatchNorm, conditioned on the 4-d action.
 *   ndp_fm_forward      replaces  forward_autoencoder(state_cur, action)   (forward_encoder.py:105-114)
 *                       training != 0: batch-statistics BatchNorm, returns the residual, moves the running
 *                       statistics when running_stats != NULL; training == 0: running statistics,
 *                       returns state_cur + residual (what control_evaluation.py / mpc_eval.py call)
 *   ndp_fm_train_grads  replaces  loss = mse(model(cur, a), fut - cur); zero_grad(); loss.backward()
 *                       (train_forward_model.py:102-109): loss[0] = the MSE, *loss_sum += it (NULL: not kept),
 *                       grad = every gradient, resid_out (NULL or [n,3,128,128]) = the prediction
 *   ndp_fm_backward     replaces  loss.backward() for ANY loss of the residual: d_resid [n,3,128,128] = d loss / d
 *                       residual; must follow ndp_fm_forward(training != 0) on the same n images with the same workspace
 *                       and nothing in between (the activations live there); grad = every gradient
 *   ndp_fm_apply_adam   replaces  optimizer.step() (:110) for the flat parameter vector, and rebuilds the
 *                       second weight order in the workspace (step_count: the Adam state word of ndp_adam_step)
 * Images [n,3,128,128] NCHW and actions [n,4] as the reference's loader delivers them.
 * Parameters are ONE flat fp32 vector (ndp_fm_param_floats() floats), gradients and Adam moments have the same
 * layout: per layer (conv1..6, deconv1..6, conv_refine_1, conv_refine_2) the weight then the bias, then per
 * BatchNorm in use (conv1..3_bn, deconv1..6_bn, conv_refine_1_bn) weight then bias.  Weights are stored
 * tap-major with the channel the kernels read along innermost, zero-padded:
 *   Conv2d           [cout_pad][kh][kw][cin_pad]   = weight.permute(0, 2, 3, 1)
 *   ConvTranspose2d  [cin_pad][kh][kw][cout_pad]   = weight.permute(0, 2, 3, 1)
 * ndp_fm_layout(what, index, &offset, dims) describes every tensor: what 0 weight / 1 bias of layer `index`
 * (dims = rows, taps, columns, kind 0 conv / 1 transposed, cin, cout), 2 / 3 BatchNorm weight / bias, 4 / 5
 * running mean / variance (offsets into the running_stats vector of ndp_fm_stat_floats() floats; dims[0] =
 * channels, dims[3] = the layer the BatchNorm follows).  Padded entries must be zero and stay zero under Adam.
 * The reference's conv4_bn / conv5_bn are never applied (forward_encoder.py:51-54) and are not part of the vector.
 * workspace: ndp_fm_workspace_floats(n) floats; its head holds the second weight order, which
 * ndp_fm_pack_params (after the parameters were written from outside) and ndp_fm_apply_adam rebuild -- the
 * same workspace pointer must be used for all calls.  ndp_fm_workspace_offset(n, t): where intermediate map t
 * (order of FmTensor in csrc/ndp_forward_model.inc) lives, for tests. */
int64_t ndp_fm_param_floats(void);
int64_t ndp_fm_stat_floats(void);
int64_t ndp_fm_workspace_floats(int64_t n_images);
int64_t ndp_fm_workspace_offset(int64_t n_images, int tensor);
int ndp_fm_layout(int what, int index, int64_t *offset, int64_t *dims /* [6] */);
int ndp_fm_pack_params(const float *params, float *workspace, void *stream);
int ndp_fm_forward(const float *params, float *running_stats, const float *state_cur,
                   const float *actions, int64_t n_images, int training, float *out,
                   float *workspace, void *stream);
int ndp_fm_train_grads(const float *params, float *running_stats, const float *state_cur,
                       const float *state_fut, const float *actions, int64_t n_images,
                       float *grad, float *loss, float *loss_sum, float *resid_out,
                       float *workspace, void *stream);
/* The weight gradients of the backward pass run on a stream of the library's own beside the caller's (fork / join by
 * events); ndp_fm_side_stream(0) keeps every launch on the caller's stream (per-kernel timing; stream capture: the fork
 * captures, but the HIP graph of it replayed at 3.9 ms against 2.0 ms eager -- and a graph of the single-stream step
 * gains nothing over eager either), returns the previous setting. */
/* ndp_fm_forward / ndp_fm_train_grads from byte frames [n][128][128][3] (see ndp_encoder_forward_u8): state_cur and
 * state_fut are normalised where they are read (the input gather and the loss), outputs are as above. */
int ndp_fm_forward_u8(const float *params, float *running_stats, const uint8_t *frames_cur,
                      const float *actions, int64_t n_images, int training, float *out,
                      float *workspace, void *stream);
int ndp_fm_train_grads_u8(const float *params, float *running_stats, const uint8_t *frames_cur,
                          const uint8_t *frames_fut, const float *actions, int64_t n_images,
                          float *grad, float *loss, float *loss_sum, float *resid_out,
                          float *workspace, void *stream);
int ndp_fm_side_stream(int on);
/* Cross-rank BatchNorm statistics for a data-parallel driver.  The per-channel sums a BatchNorm needs are accumulated
 * by the kernel that produces its input as 64-bit fixed-point integers (csrc/ndp_forward_model.inc, "epilogue
 * statistics").  A *_train_grads_dp call given such a function invokes fn(acc, words, stream, ctx) on the calling
 * thread between the launch that fills an accumulator and the launch that reads it; fn must enqueue, on `stream`, an
 * in-place SUM over the ranks of the `words` int64 values at `acc` (device memory inside the workspace) -- an RCCL
 * all-reduce of ncclInt64.  Integer sums are exact and order-free: `world` ranks with B / world images each then
 * normalise, and update the running statistics, exactly as one process with B images does (the reference trains on one
 * device: train_forward_model.py:62); the BatchNorm weight / bias gradients stay each rank's own share, for the gradient
 * all-reduce to add up.  fn == NULL: off (per-rank statistics, what torch's DistributedDataParallel does without
 * SyncBatchNorm).  The function travels with the call: the library keeps no pointer to it once the call has returned. */
typedef void (*ndp_fm_stat_sync_fn)(void *acc, int64_t words, void *stream, void *ctx);
/* Data parallel: ndp_fm_train_grads (frames_u8 == 0: float frames) or ndp_fm_train_grads_u8 (frames_u8 != 0) for one
 * rank's share of a global batch -- the same launches, the same bits -- with the 10 BatchNorms' statistics summed over
 * `world` ranks through stat_sync (10 forward + 10 backward calls: 20 small collectives per iteration).  stat_sync ==
 * NULL or world == 1: this rank's statistics only (1 <= world <= 4096, else NDP_E_ARG and nothing launched).  No other
 * ndp_fm_* entry point sums statistics over ranks: ndp_fm_forward / ndp_fm_backward(_inputs) take no function. */
int ndp_fm_train_grads_dp(const float *params, float *running_stats, const void *frames_cur, const void *frames_fut,
                          int frames_u8, const float *actions, int64_t n_images, float *grad, float *loss,
                          float *loss_sum, float *resid_out, float *workspace, void *stream,
                          ndp_fm_stat_sync_fn stat_sync, void *stat_ctx, int world);

/* Gradient buckets for a data-parallel driver (the reference trains on one device: train_forward_model.py:62; the
 * north star asks for the all-reduce of the gradients "overlapped with backward").  ndp_fm_grad_buckets writes the 7
 * ranges (offset, count: floats of the flat gradient) in the order in which a backward pass completes them -- the weight
 * gradients come last layer first -- and returns 7.  Every ndp_fm_train_grads / ndp_fm_backward call records one event
 * per bucket where its last byte is written; ndp_fm_bucket_wait(b, stream) makes `stream` (the caller's communication
 * stream) wait for bucket b of the most recent such call on the current device, so that its all-reduce runs beside the
 * rest of the backward pass (NDP_E_ARG before the first one).  The buckets cover the whole vector exactly once. */
int ndp_fm_grad_buckets(int64_t *offsets, int64_t *counts, int capacity);
int ndp_fm_bucket_wait(int bucket, void *stream);
int ndp_fm_backward(const float *params, const float *d_resid, int64_t n_images, float *grad,
                    float *workspace, void *stream);
int ndp_fm_apply_adam(float *params, const float *grad, float *exp_avg, float *exp_avg_sq,
                      int32_t *step_count, float lr, float beta1, float beta2, float eps,
                      float *workspace, void *stream);
/* Input gradients of the EVAL-mode forward pass (out = state_cur + residual, BatchNorm with the running statistics):
 * d_out [n,3,128,128] = d loss / d out  ->  d_state_cur [n,3,128,128] (or NULL) and d_actions [n,4] (or NULL; not both).
 * Must follow ndp_fm_forward / ndp_fm_forward_u8 (training == 0) on the same n images with the same workspace and no
 * other ndp_fm_* call on that workspace in between; it consumes the activations, so a second call (or one without such
 * a forward pass) returns NDP_E_UNSUPPORTED and launches nothing.  Only the data-gradient chain runs -- no parameter
 * gradient is written anywhere -- and with d_state_cur == NULL it stops at the decoder's first layer. */
int ndp_fm_input_grads(const float *params, const float *d_out, int64_t n_images,
                       float *d_state_cur, float *d_actions, float *workspace, void *stream);

/* The eval-mode pass with a choice of operand precision (the planner's passes: it ranks sampled rollouts by a pixel MSE
 * and tolerates operand rounding; training and every other entry point stay fp32).
 *   NDP_FM_FP32  the launches and the bits of ndp_fm_forward / ndp_fm_forward_u8 (training == 0); lp_weights may be NULL.
 *   NDP_FM_BF16  changes exactly this: layers 1..4 and 7..11 (conv2..conv5, deconv2..deconv6: the stride-2 layers, 99 % of
 *                the multiplications) compute  out = act(bias + sum bf16(x) * bf16(w))  where bf16(.) rounds fp32 to bf16
 *                to nearest even (NaN stays NaN, overflow goes to +-Inf), a product of two bf16 values is exact in fp32,
 *                and the sum is accumulated in fp32 (the accumulator of v_mfma_f32_16x16x32_bf16; K-split partial sums and
 *                their reduction stay fp32).  Bias, activation, BatchNorm with the running statistics, the skip
 *                concatenations and every stored map stay fp32 -- the workspace layout is unchanged -- and conv1, conv6,
 *                deconv1 and the refinement stage keep their fp32 kernels.  The activations are rounded where a kernel
 *                stages them; the weights are rounded ONCE: ndp_fm_pack_params_lp writes, into a caller-owned buffer of
 *                ndp_fm_lp_weight_bytes() bytes (16-byte aligned), the bf16 copy of the weight order each of the nine
 *                layers' forward launch reads (a convolution's first, a transposed convolution's second), one launch.
 *                It reads `params` and the second weight order in the workspace head, so it follows ndp_fm_pack_params
 *                / ndp_fm_apply_adam on the same stream whenever the parameters change.
 * Exactly one of state_cur (float [n,3,128,128]) and frames_u8 (bytes [n][128][128][3]) is given.  Any other precision,
 * NDP_FM_BF16 without lp_weights, both or neither image pointer: NDP_E_ARG, nothing launched.  A bf16 pass leaves no
 * activations that ndp_fm_input_grads may consume: after it that call returns NDP_E_UNSUPPORTED and launches nothing.
 * Two passes on the same inputs give the same bits (fixed-order sums, as everywhere). */
#define NDP_FM_FP32 0
#define NDP_FM_BF16 1
int64_t ndp_fm_lp_weight_bytes(void);
int ndp_fm_pack_params_lp(const float *params, const float *workspace, void *lp_weights, void *stream);
int ndp_fm_forward_lp(const float *params, const float *running_stats, const float *state_cur,
                      const uint8_t *frames_u8, const float *actions, int64_t n_images, int precision,
                      const void *lp_weights, float *out, float *workspace, void *stream);

/* The image encoder's pass with the same choice (the planner encodes every predicted frame once per horizon step).
 *   NDP_ENC_FP32  the launches and the bits of ndp_encoder_forward / ndp_encoder_forward_u8; lp_weights may be NULL.
 *   NDP_ENC_BF16  differs in exactly these points:
 *     - conv2..conv6 compute  out = act(bias + sum bf16(x) * bf16(w))  with w the packed fp32 weight (BatchNorm folded
 *       in), bf16(.) fp32 -> bf16 to nearest even (NaN stays NaN, overflow goes to +-Inf), products exact in fp32, the sum
 *       in fp32 (the accumulator of v_mfma_f32_16x16x32_bf16), the bias fp32, ReLU applied in fp32;
 *     - conv1 keeps its fp32 arithmetic on the image and on its fp32 weights;
 *     - the maps behind conv1..conv5 are STORED as bf16: the rounding of the next layer's operand, done once by the
 *       producer (each map is read by the next convolution only).  K-split partial sums and the codes stay fp32;
 *     - a ReLU passes a NaN on (the fp32 pass's maximum with zero drops it), so a NaN pixel gives that image NaN codes;
 *     - the weights are rounded ONCE: ndp_encoder_pack_params_lp writes the bf16 copy of conv2..conv6's packed weights,
 *       in the same [Cout][KH][KW][Cin] order, back to back, into a caller-owned buffer of ndp_encoder_lp_weight_bytes()
 *       bytes (2 * 8,364,032; 16-byte aligned), one launch; it follows every change of packed_params.
 * Workspace: ndp_encoder_workspace_floats(n) serves both precisions.  A bf16 pass of c <= 512 images lays out the five
 * maps, consecutive, as bf16, NHWC ([c][64][64][64], [c][32][32][128], [c][16][16][256], [c][8][8][512], [c][4][4][1024]),
 * then the fp32 partial sums; ndp_encoder_lp_act_offset(layer 0..4, n_images) (host only) is a map's offset in bf16
 * elements for c = min(n_images, 512), -1 for any other layer or n_images < 1.  Passes reuse the workspace, so after a
 * call the maps are those of the last pass.
 * Exactly one of images (float [n,3,128,128]) and frames_hwc (bytes [n][128][128][3]) is given.  An unknown precision,
 * NDP_ENC_BF16 without lp_weights, both or neither image pointer, a buffer that is not 16-byte aligned (packed_params, images,
 * lp_weights, codes, workspace; frames_hwc may have any alignment, as in ndp_encoder_forward_u8), n_images < 1: NDP_E_ARG,
 * nothing launched.  Two passes on the same inputs give the same bits; byte frames and the floats built from them too. */
#define NDP_ENC_FP32 0
#define NDP_ENC_BF16 1
int64_t ndp_encoder_lp_weight_bytes(void);
int64_t ndp_encoder_lp_act_offset(int layer, int64_t n_images);
int ndp_encoder_pack_params_lp(const float *packed_params, void *lp_weights, void *stream);
int ndp_encoder_forward_lp(const float *packed_params, const float *images, const uint8_t *frames_hwc,
                           int64_t n_images, int precision, const void *lp_weights, float *codes,
                           float *workspace, void *stream);

/* ndp_fm_backward with the gradient of the TRAINING-mode pass with respect to its inputs as well: the same precondition
 * (a training-mode ndp_fm_forward on this workspace came first), the same launches and bit for bit the same `grad`, plus
 * d_state_cur [n,3,128,128] (or NULL) = d loss / d state_cur through the network alone -- the training-mode output is
 * the residual, so there is no identity term; a caller that forms state_cur + residual adds it -- and d_actions [n,4]
 * (or NULL).  One more launch on the caller's stream, beside the last weight gradient. */
int ndp_fm_backward_inputs(const float *params, const float *d_resid, int64_t n_images, float *grad,
                           float *d_state_cur, float *d_actions, float *workspace, void *stream);
/* Multi-step rollout training: for a window of H + 1 frames x_0 .. x_H and H actions per trajectory,
 *   s_0 = x_0;  r_k = model(s_k, a_k) in training mode;  s_{k+1} = s_k + r_k (not detached);
 *   loss_k = mean((s_{k+1} - x_{k+1})^2);  L = (loss_0 + .. + loss_{H-1}) / H
 * and the gradient of L through every path.  The caller keeps one workspace per pass (each needs ndp_fm_pack_params
 * after every ndp_fm_apply_adam: the second weight order lives in the workspace's head), runs ndp_fm_forward(training)
 * on s_k for k = 0 .. H-1 with ndp_fm_rollout_advance behind each, then for k = H-1 .. 0 ndp_fm_backward_inputs with
 * d_resid = G_{k+1} and, for k >= 1, ndp_fm_rollout_chain; ndp_fm_grad_sum adds the H gradients.  With N = n*3*128*128:
 *   ndp_fm_rollout_begin    state = x_0 as contiguous floats.  frames: image i at frames + i * image_stride ELEMENTS
 *                           (floats [3][128][128], or with frames_u8 != 0 bytes [128][128][3], normalised as
 *                           ndp_encoder_forward_u8 describes: the floats the loader would upload, bit for bit)
 *   ndp_fm_rollout_advance  state_next = state + resid;  local_next = (2 / (H N)) (state_next - target) = local_{k+1};
 *                           step_losses[step] = loss_step;  loss[0] = (step == 0 ? 0 : loss[0]) + loss_step / steps;
 *                           after the last step *loss_sum += loss[0] (NULL: not kept).  target: as `frames` above.
 *                           workspace: that of pass `step` (its loss scratch holds the blocks' sums)
 *   ndp_fm_rollout_chain    g = (local + g_next) + d_state_cur = G_k, elementwise over [n,3,128,128]; g may be `local`
 *   ndp_fm_grad_sum         out = ((g_0 + g_1) + ..) + g_{count-1}, vector h at grads + h * stride, `floats` long
 * Every sum is taken in one fixed order (squares in fp64, no float atomics): two runs give the same bits.  All launches
 * go to `stream`. */
int ndp_fm_rollout_begin(const void *frames, int frames_u8, int64_t image_stride, int64_t n_images,
                         float *state, void *stream);
int ndp_fm_rollout_advance(const float *state, const float *resid, const void *target, int target_u8,
                           int64_t image_stride, int64_t n_images, int step, int steps,
                           float *state_next, float *local_next, float *step_losses, float *loss,
                           float *loss_sum, float *workspace, void *stream);
int ndp_fm_rollout_chain(const float *local, const float *g_next, const float *d_state_cur,
                         int64_t n_images, float *g, void *stream);
int ndp_fm_grad_sum(const float *grads, int64_t stride, int count, int64_t floats, float *out, void *stream);

/* ------------------------------------------------------- image autoencoder ---
 * models.image_autoencoder.Encoder + Decoder (image_autoencoder.py:14-87) and one iteration of their training loop
 * (train_autoencoder.py:79-90).  Additive to the forward-model family above, same conventions:
 *   ndp_ae_train_grads  replaces  recon = decoder(encoder(x)); loss = mse(recon, x); zero_grad(); loss.backward()
 *                       images [n,3,128,128] NCHW; training-mode BatchNorm (batch statistics; the running statistics
 *                       move when running_stats != NULL); loss[0] = the MSE, *loss_sum += it (NULL: not kept);
 *                       grad = every gradient; recon_out (NULL or [n,3,128,128]) = the reconstruction
 *   ndp_ae_apply_adam   replaces  optimizer.step() (:90) for the flat parameter vector and rebuilds the second weight
 *                       order in the workspace (step_count: the Adam state word of ndp_adam_step)
 * Parameters: ONE flat fp32 vector of ndp_ae_param_floats() floats, per layer (conv1..6, deconv1..6) the weight then
 * the bias, then per BatchNorm in use (conv1..3_bn, deconv1..5_bn) weight then bias; weights as in the forward model
 * (Conv2d [cout_pad][kh][kw][cin_pad], ConvTranspose2d [cin_pad][kh][kw][cout_pad]; conv1's cin 3 -> 32, deconv6's
 * cout 3 -> 4).  ndp_ae_layout: as ndp_fm_layout (what 0..5) over this vector and the running_stats vector of
 * ndp_ae_stat_floats() floats.  conv4_bn / conv5_bn are never applied (image_autoencoder.py:42-45) and are not part of
 * the vectors.  workspace: ndp_ae_workspace_floats(n) floats, the same pointer for every call; its head holds the
 * second weight order, which ndp_ae_pack_params (after the parameters were written from outside) and
 * ndp_ae_apply_adam rebuild.  1 <= n_images <= 8192 (larger: NDP_E_ARG; ndp_ae_workspace_floats returns 0).
 * ndp_ae_workspace_offset(n, t): where intermediate map t (order of AeTensor in csrc/ndp_autoencoder.inc) lives, for
 * tests; -1 for a bad query. */
int64_t ndp_ae_param_floats(void);
int64_t ndp_ae_stat_floats(void);
int64_t ndp_ae_workspace_floats(int64_t n_images);
int64_t ndp_ae_workspace_offset(int64_t n_images, int tensor);
int ndp_ae_layout(int what, int index, int64_t *offset, int64_t *dims /* [6] */);
int ndp_ae_pack_params(const float *params, float *workspace, void *stream);
int ndp_ae_train_grads(const float *params, float *running_stats, const float *images, int64_t n_images,
                       float *grad, float *loss, float *loss_sum, float *recon_out, float *workspace,
                       void *stream);
int ndp_ae_apply_adam(float *params, const float *grad, float *exp_avg, float *exp_avg_sq,
                      int32_t *step_count, float lr, float beta1, float beta2, float eps,
                      float *workspace, void *stream);
/* Data parallel: ndp_ae_train_grads for one rank's share of a global batch, with
 *   - cross-rank BatchNorm statistics through the function given with THIS call (ndp_fm_stat_sync_fn: same contract as
 *     ndp_fm_train_grads_dp's): the 8 BatchNorms call stat_sync(acc, words, stream, stat_ctx)
 *     between the launch that fills an accumulator and the launch that reads it, 8 forward + 8 backward calls; the
 *     running statistics and dx come from the sums over the ranks, d gamma / d beta from this rank's own.
 *     stat_sync == NULL or world == 1: this rank's statistics only (1 <= world <= 4096);
 *   - gradient buckets: ndp_ae_grad_buckets writes the 6 ranges (offset, count: floats of the flat gradient) in the
 *     order the backward pass completes them -- deconv3..6, deconv2, deconv1 + conv6, conv5, conv1..4, the BatchNorm
 *     weights and biases; they cover the vector exactly once -- and the count through n_buckets (NDP_OK, or an error
 *     code and nothing written).  Every ndp_ae_train_grads_dp call records one event per bucket where its last byte is
 *     written; ndp_ae_bucket_wait(b, stream) makes `stream` wait for bucket b of the most recent such call on the current
 *     device (NDP_E_ARG before the first one).  The gradient bits are those of ndp_ae_train_grads. */
int ndp_ae_train_grads_dp(const float *params, float *running_stats, const float *images, int64_t n_images,
                          float *grad, float *loss, float *loss_sum, float *recon_out, float *workspace,
                          void *stream, ndp_fm_stat_sync_fn stat_sync, void *stat_ctx, int world);
int ndp_ae_grad_buckets(int64_t *offsets, int64_t *counts, int capacity, int *n_buckets);
int ndp_ae_bucket_wait(int bucket, void *stream);

/* Eval-mode Decoder (image_autoencoder.py:80-87 under .eval()) and reconstruction error.  The five BatchNorms are folded
 * into the transposed convolutions ON THE HOST, in fp32: scale = gamma / sqrt(running_var + 1e-5), w' = w * scale[cout],
 * b' = (b - running_mean) * scale + beta (models/image_autoencoder.py: fold_decoder_params); the kernels never read a
 * BatchNorm tensor and launch no BatchNorm kernel.  folded_params: ndp_ae_decoder_param_floats() floats, deconv1..6, per
 * layer the weight [cin_pad][kh][kw][cout_pad] then the bias [cout_pad] (deconv6's cout 3 -> 4); ndp_ae_decoder_layout:
 * as ndp_fm_layout with what 0 / 1 (this network has no BatchNorm: what 2..5 is NDP_E_ARG).
 * workspace: ndp_ae_decode_workspace_floats(n) floats (0 for n < 1); it grows with n only up to
 * ndp_ae_decode_pass_images() images, the pass size in which ndp_ae_decode walks a larger batch.  Its head holds the
 * second weight order of deconv1..5: call ndp_ae_decode_pack whenever folded_params changed or the workspace is new.
 *   ndp_ae_decode   codes [n,128] -> recon_f32 [n,3,128,128] (NCHW, or NULL) and / or recon_u8 [n,128,128,3] (HWC bytes,
 *                   trunc(((y + 1) / 2) * 255) in fp32: the reference's denorm(...).astype(np.uint8),
 *                   train_autoencoder.py:42-43, 97-100; or NULL).  With ONE target -- target_f32 [n,3,128,128] or
 *                   target_u8 [n,128,128,3] byte frames, normalised as the loader does, (b / 255 - 0.5) * 2 --
 *                   sq_err[i] (or NULL) = the mean squared error of image i over its 49,152 values and mean_err[0] (or
 *                   NULL) = the mean of sq_err over the batch.  Fixed summation order, no float atomics: two calls give
 *                   the same bits.  Two targets, sq_err / mean_err without a target, no output at all, n < 1: NDP_E_ARG,
 *                   nothing launched.  Float buffers 16-byte aligned, byte buffers 4-byte aligned. */
int64_t ndp_ae_decoder_param_floats(void);
int ndp_ae_decoder_layout(int what, int index, int64_t *offset, int64_t *dims /* [6] */);
int64_t ndp_ae_decode_workspace_floats(int64_t n_images);
int64_t ndp_ae_decode_pass_images(void);
int ndp_ae_decode_pack(const float *folded_params, float *workspace, void *stream);
int ndp_ae_decode(const float *folded_params, const float *codes, int64_t n_images, float *recon_f32,
                  unsigned char *recon_u8, const float *target_f32, const unsigned char *target_u8,
                  float *sq_err, float *mean_err, float *workspace, void *stream);

/* ------------------------------------------------------------- evaluation ---
 * The glue of the evaluation scripts (control_evaluation.py, complete_eval.py, mpc_eval.py) between the encoder, the
 * generator and the forward model (csrc/ndp_eval.inc).  Images are `values` contiguous floats each (3*128*128 for the
 * scripts' images).  Every reduction runs in a fixed order without float atomics: results are bit-reproducible.
 *   ndp_eval_score_select  replaces  mpc_eval.py:158-169: err_now = mse(state_fut_hat[ro], state_target[0]) per rollout,
 *                          the `if err_now < min_error` loop (:129, :159-165: sentinel 10000000000, strict `<` in
 *                          rollout order, so the first minimum wins, a NaN error is never chosen and rollout 0 stands
 *                          when no error is below the sentinel; one host sync per rollout there, none here),
 *                          best_action_so_far = action_now_taken[best] (:165), and the extra forward-model call of
 *                          :167-169, whose result is the chosen rollout's ts = 0 prediction (copied from pred0).
 *                          pred [n_traj * rollouts] rows trajectory-major; pair p is scored against
 *                          target[target_idx ? target_idx[p] : p / rollouts]; err [n_traj*rollouts] = the pair's MSE
 *                          (mean of `values` squares, summed in fp64, rounded to fp32); choice [n_traj] int32;
 *                          action_out [n_traj,4] = actions0 [n_traj*rollouts,4] at the choice; pred_out [n_traj,values]
 *                          = pred0 at the choice (pred0 / pred_out: both or neither).  forced: NULL, or [n_traj] indices
 *                          that replace the rule (an index outside 0..rollouts-1 falls back to the rule).
 *   ndp_eval_mse           replaces  image_error = mse(state_fut_hat, state_fut); image_error_sum += image_error
 *                          (control_evaluation.py:132-135, complete_eval.py:141-144, mpc_eval.py:173-176) and
 *                          action_error = mse(...); action_error_sum += action_error (:137-142 / :146-151 / :180-184):
 *                          pair p compares a[a_idx ? a_idx[p] : p] with b[b_idx ? b_idx[p] : p]; each `group`
 *                          consecutive pairs form one MSE (mean over group * values squares, fp64, rounded to fp32):
 *                          mse [n_pairs/group] (may be NULL), and acc [n_pairs/group] (may be NULL) += it in fp32, the
 *                          reference's accumulation order.  A pair whose index is out of range gives NaN.
 *                          ws: ndp_eval_mse_ws_floats(n_pairs) floats, 8-byte aligned.
 *   ndp_eval_g_input       replaces  torch.cat([state_codes, target_codes], dim=1).squeeze() with the goal encoded R x Th
 *                          times (mpc_eval.py:131-141; control_evaluation.py:104-112): out [rows,256] row r =
 *                          cat(state_code[r / state_rep], goal_code[r / goal_rep]), codes [n,128] -- the code input of
 *                          ndp_g_forward (ld_code 256)
 *   ndp_eval_frames_u8     replaces  the host-side normalisation of the loader's frames (utils/hdf5_load.py:9-11):
 *                          frames_hwc [n][128][128][3] bytes -> images [n,3,128,128] in [-1,1], with the 256-entry table
 *                          of ndp_encoder_forward_u8 (bit-identical to the float path).
 *   ndp_fm_score           scores n predictions of the eval-mode forward model, pred [n,3,128,128] (= state_cur +
 *                          residual, the output of ndp_fm_forward(training = 0)), in ONE launch (forward_model_eval.py):
 *                          - pred_err [n] (or NULL): the MSE of prediction i over its 49,152 values against target row
 *                            target_idx ? target_idx[i] : i of EXACTLY ONE of target_f32 [n_target,3,128,128] and
 *                            target_u8 [n_target,128,128,3] (byte frames, normalised through the table of
 *                            ndp_eval_frames_u8: the bits of the floats of the same bytes).  The difference is taken in
 *                            fp32, its square summed in fp64 in a fixed order, the mean rounded to fp32;
 *                          - base_err [n] (required with a base frame, else NULL): the same MSE between base row
 *                            base_idx ? base_idx[i] : i of base_f32 [n_base,3,128,128] or base_u8 [n_base,128,128,3] (at
 *                            most one) and the same target: the error of predicting "the frame does not change";
 *                          - pred_u8 [n,128,128,3] (or NULL): HWC bytes trunc(((y + 1) / 2) * 255), the fp32 operations
 *                            of ndp_ae_decode in the same order -- the reference's denorm(...).astype(np.uint8),
 *                            train_forward_model.py:116-145.  DEVIATION: state + residual can leave [-1, 1]; values
 *                            below 0 / from 255 up are written as 0 / 255 and NaN as 0, where numpy's cast wraps.
 *                          An index outside its array gives NaN for that image's error (base_err also where the target
 *                          index is bad) and nothing is read through it; the bytes do not depend on the indices.  No gathered
 *                          copy, no scratch, no atomics: two calls give the same bits.  Two targets, no target, two base
 *                          frames, a base frame without base_err (or base_err / base_idx without one), no output at all,
 *                          n < 1 or n_target < 1: NDP_E_ARG, nothing launched.  Float images 16-byte aligned, byte
 *                          frames 4-byte aligned.  The caller owns every buffer.
 *   ndp_gan_score          scores n conditioning rows of K samples of the action generator, action_hat [n,K,4] (what
 *                          ndp_g_forward writes for m = n * K rows with code_rep = K), in ONE launch (gan_eval.py).  Inputs
 *                          (device pointers): action [n,4] the true actions, or NULL; noise [n,K,nz], or NULL (nz is read
 *                          only with it); fake_logits [n,K] = ndp_d_forward on the samples, or NULL.  Outputs, each may be
 *                          NULL, at least one required; e_k is the error of sample k:
 *                          - sample_err [n,K]: e_k = the mean of the 4 squares of the fp32 differences between sample k
 *                            and the true action, summed in fp64 in index order, rounded to fp32 (ndp_fm_score's
 *                            convention);
 *                          - mean_err [n]: the mean over all K * 4 squares, fp64 sum in (k, component) order, rounded
 *                            once; its mean over rows is mse(repeat_interleave(actions, K), action_hat)
 *                            (control_evaluation.py:140-142);
 *                          - best_err [n], best_k [n] int32: the smallest e_k, the first minimum wins; a NaN e_k is never
 *                            chosen while a non-NaN one exists; all NaN: k = 0 and NaN;
 *                          - best_curve [n,K]: the running minimum over samples 0 .. k under the same rule (its mean over
 *                            rows is the best-of-(k + 1) curve);
 *                          - spread [n]: the mean over the K (K - 1) ordered pairs i != j of ||a_i - a_j||_2 (fp32
 *                            distances as ndp_ndiv_fwd_bwd takes them, summed in fp64 per sample i over j, then over i);
 *                            K = 1: NaN (0/0);
 *                          - ndiv [n] (needs noise): the row's share of ndp_ndiv_fwd_bwd's loss, sum_{i,j} relu(0.8 *
 *                            dz_ij / sum_j dz_ij - dx_ij / sum_j dx_ij), every term in fp32 in that kernel's operation
 *                            order (fmaf chains, sqrtf, fp32 row sums in j order, a separately rounded product and
 *                            difference), NaN propagating as there; the K terms of sample i are summed in fp64 in j
 *                            order, the K subtotals in i order, rounded once;
 *                          - d_fake_prob [n] (needs fake_logits): the mean over k of sigmoid(logit), the sigmoid in the
 *                            form the BCE kernels use, 1 / (1 + expf(-x)) in fp32, summed in fp64 in k order;
 *                          - d_pick_k [n] int32 (needs fake_logits), d_pick_err [n] (needs action too): the sample with
 *                            the largest logit (first maximum, NaN never chosen; all NaN: 0) and its e_k.
 *                          1 <= K <= NDP_MAX_SAMPLES, 1 <= nz <= 16, n >= 1, n * K < 2^31.  An output without the input
 *                          it needs, no output at all, a limit exceeded: NDP_E_ARG, nothing launched.  No scratch buffer,
 *                          no atomics (two calls give the same bits), no host synchronisation.  The caller owns every
 *                          buffer.
 *   ndp_image_quality      SSIM and PSNR of n_pairs image pairs (image_quality.py; nothing in the reference computes
 *                          either).  Pair p compares a[a_idx ? a_idx[p] : p] with b[b_idx ? b_idx[p] : p]; each side is
 *                          EXACTLY ONE of floats [n,3,128,128] in [-1, 1] and byte frames [n,128,128,3] (through the
 *                          table of ndp_eval_frames_u8: the bits of the floats of the same bytes).
 *                          - scale: u = (x + 1) * 0.5 in fp32, clamped to [0, 1] (-Inf -> 0, +Inf -> 1); a NaN stays
 *                            NaN and makes both results of its pair NaN;
 *                          - psnr [n_pairs] (or NULL): the fp32 differences of u, their squares summed in fp64 in a fixed
 *                            order, mse = sum / 49152, 10 * log10(1 / mse) in fp64 rounded to fp32; mse == 0: +Inf;
 *                          - ssim [n_pairs] (or NULL): Wang et al. 2004 as scikit-image computes it with
 *                            gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=1: per channel an
 *                            11-tap separable Gaussian g[i] ~ exp(-(i-5)^2 / (2 * 1.5^2)) (normalised in double, rounded
 *                            to fp32 once) over the windows wholly inside the image (118 x 118 positions) gives ux, uy,
 *                            uxx, uyy, uxy of x, y, x*x, y*y, x*y; vx = uxx - ux*ux, vy = uyy - uy*uy, vxy = uxy - ux*uy;
 *                            S = ((2 ux uy + C1)(2 vxy + C2)) / ((ux ux + uy uy + C1)(vx + vy + C2)), C1 = 0.01^2,
 *                            C2 = 0.03^2; the mean of the 3 * 118 * 118 values of S, summed in fp64 in a fixed order,
 *                            rounded to fp32 once.  Filtering and S are fp32, in an operation order that gives an image
 *                            against itself exactly 1.0f.
 *                          An index outside its array gives NaN for both results of that pair; nothing is read through
 *                          it.  workspace: ndp_image_quality_ws_bytes(n_pairs) bytes (0 for a bad request), 8-byte
 *                          aligned; float images 16-byte aligned.  Both or neither pointer of a side, no output,
 *                          n_pairs < 1, n_a < 1, n_b < 1, a workspace that is too small: NDP_E_ARG, nothing launched.
 *                          No atomics, no host synchronisation; two calls give the same bits, and the result does not
 *                          depend on how the rows are split over workgroups.  The caller owns every buffer. */
int ndp_eval_score_select(const float *pred, int64_t n_traj, int rollouts, const float *target, int64_t n_target,
                          const int32_t *target_idx, int64_t values, const float *actions0, const float *pred0,
                          const int32_t *forced, float *err, int32_t *choice, float *action_out, float *pred_out,
                          void *stream);
int64_t ndp_eval_mse_ws_floats(int64_t n_pairs);
int ndp_eval_mse(const float *a, int64_t n_a, const float *b, int64_t n_b, const int32_t *a_idx, const int32_t *b_idx,
                 int64_t n_pairs, int64_t values, int64_t group, float *mse, float *acc, float *ws, void *stream);
int ndp_eval_g_input(const float *state_code, int64_t n_state, int state_rep, const float *goal_code, int64_t n_goal,
                     int goal_rep, int64_t rows, float *out, void *stream);
int ndp_eval_frames_u8(const uint8_t *frames_hwc, int64_t n_images, float *images, void *stream);
int ndp_fm_score(const float *pred, int64_t n_images, const float *target_f32, const uint8_t *target_u8,
                 int64_t n_target, const int32_t *target_idx, const float *base_f32, const uint8_t *base_u8,
                 int64_t n_base, const int32_t *base_idx, float *pred_err, float *base_err, uint8_t *pred_u8,
                 void *stream);
int ndp_gan_score(const float *action_hat, int64_t n, int k, const float *action, const float *noise, int nz,
                  const float *fake_logits, float *sample_err, float *mean_err, float *best_err, int32_t *best_k,
                  float *best_curve, float *spread, float *ndiv, float *d_fake_prob, int32_t *d_pick_k,
                  float *d_pick_err, void *stream);
int64_t ndp_image_quality_ws_bytes(int64_t n_pairs);
int ndp_image_quality(const float *a_f32, const uint8_t *a_u8, int64_t n_a, const int32_t *a_idx, const float *b_f32,
                      const uint8_t *b_u8, int64_t n_b, const int32_t *b_idx, int64_t n_pairs, float *ssim, float *psnr,
                      void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------- JPEG decode ---
 * The frames of the reference's trajectory bundles are JPEG streams (generate_trajectories.py:113-122: PIL, quality 95);
 * ndp_jpeg_decode_u8 turns a batch of them into the [n][128][128][3] bytes that the *_u8 entry points take, bit-identical
 * to PIL (libjpeg-turbo: integer islow IDCT, "fancy" h2v2 chroma upsampling, fixed-point YCbCr -> RGB).
 * Supported: baseline / extended sequential DCT (SOF0 / SOF1), 8-bit, Huffman, one interleaved scan, 3 components
 * sampled 4:2:0 (Y 2x2, Cb 1x1, Cr 1x1) with Cb and Cr sharing their Huffman tables, 128x128; any DQT / DHT tables;
 * 0xFF00 stuffing, fill bytes, APPn / COM segments.  Anything else is not decoded and gets a status:
 *   streams     device bytes; frame i is streams[offsets[i] .. offsets[i+1]) (offsets: n+1 device int64, non-decreasing);
 *               nothing outside that range is read for frame i
 *   frames_hwc  [n][128][128][3] bytes; a frame whose status is not NDP_JPEG_OK is all zero
 *   status      [n] int32, one of NDP_JPEG_*
 *   workspace   ndp_jpeg_workspace_bytes(n, stream_bytes) bytes, 256-byte aligned, where stream_bytes >=
 *               offsets[n] - offsets[0]; a frame that does not fit a smaller workspace gets NDP_JPEG_WORKSPACE.
 * No host synchronisation: the host never reads the streams or the offsets.  1 <= n_images <= 65536;
 * ndp_jpeg_workspace_bytes returns 0 for a bad request. */
#define NDP_JPEG_OK          0
#define NDP_JPEG_UNSUPPORTED 1   /* progressive, arithmetic, 12-bit, restart intervals, not 3 components at 4:2:0, ... */
#define NDP_JPEG_SIZE        2   /* not 128x128 */
#define NDP_JPEG_CORRUPT     3   /* corrupt or truncated stream (bad marker, segment past the end, bad Huffman code,
                                    entropy data shorter than the 384 blocks, no EOI) */
#define NDP_JPEG_WORKSPACE   4   /* the stream does not fit the workspace's stream area */
int64_t ndp_jpeg_workspace_bytes(int64_t n_images, int64_t stream_bytes);
int ndp_jpeg_decode_u8(const uint8_t *streams, const int64_t *offsets /* [n+1], device */, int64_t n_images,
                       uint8_t *frames_hwc /* [n][128][128][3] */, int32_t *status /* [n], device */, void *workspace,
                       int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------- JPEG encode ---
 * The reference writes every camera frame with PIL: im.save(format="jpeg", quality=95) (generate_trajectories.py:
 * 113-122).  ndp_jpeg_encode_u8 writes the same bytes on the device: baseline, 8-bit, 128x128, 4:2:0, the Annex K
 * quantisation tables scaled for quality 95, the standard Huffman tables, no restart markers; libjpeg's fixed-point
 * colour conversion, h2v2 box downsampling, integer islow forward DCT and sign-magnitude quantisation.  Exact for every
 * pixel array, not only camera-like ones.  The output is what ndp_jpeg_decode_u8 reads.
 *   frames_hwc  [n][128][128][3] device bytes, 4-byte aligned
 *   streams     device bytes: frame i is streams[offsets[i] .. offsets[i+1]), offsets[0] = 0; nothing is written at or
 *               beyond streams + capacity
 *   offsets     [n+1] device int64 (written)
 *   status      [n] device int32: NDP_JPEG_OK, or NDP_JPEG_WORKSPACE for the first frame that does not fit in what is
 *               left of `capacity` and for every frame after it (their length is 0; the frames before are intact)
 *   workspace   ndp_jpeg_encode_workspace_bytes(n) bytes, 256-byte aligned (0 for a bad request).  After the call the
 *               n int64 at byte ndp_jpeg_encode_lengths_offset(n) of it (-1 for a bad n; host only) are the stream
 *               lengths of all n frames, of those that did not fit too: their sum is the capacity that fits the batch
 * ndp_jpeg_encode_max_stream_bytes (host only): the longest stream a frame can give -- header, the entropy bound
 * derived from the Huffman tables with every byte stuffed, EOI; capacity = n * that always fits.
 * No host synchronisation, no allocation; 1 <= n_images <= 65536.  Integer arithmetic, atomics in LDS only (OR): two
 * runs give the same bytes. */
int64_t ndp_jpeg_encode_workspace_bytes(int64_t n_images);
int64_t ndp_jpeg_encode_max_stream_bytes(void);
int64_t ndp_jpeg_encode_lengths_offset(int64_t n_images);
int ndp_jpeg_encode_u8(const uint8_t *frames_hwc, int64_t n_images, uint8_t *streams, int64_t capacity,
                       int64_t *offsets /* [n+1], device */, int32_t *status /* [n], device */, void *workspace,
                       int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------- Lanczos resize ---
 * A live environment renders camera frames of any size (MuJoCo: 500x500); the reference turns them into the networks'
 * input with PIL: Image.fromarray(frame).resize((128, 128), Image.LANCZOS) (MPC_gym_eval.py:68-77,
 * generate_trajectories.py:113-118).  ndp_resize_lanczos_u8 does that on the device, bit-identical to Pillow's 8-bit
 * resampler (fixed-point coefficients with 22 fractional bits, horizontal pass rounded to bytes, then the vertical pass;
 * a pass whose input size is 128 is skipped, so a 128x128 frame is copied).
 *   ndp_resize_workspace_bytes(H, W)  bytes of the coefficient tables of one frame size; 0 unless 1 <= H, W <= 2048
 *   ndp_resize_build_tables           host only, no GPU call: fills `tables_host` (4-byte aligned, `bytes` >= the above)
 *                                     in double arithmetic.  The caller copies the tables to device memory once per
 *                                     (H, W) and owns them.
 *   ndp_resize_lanczos_u8             frames_hwc [n][H][W][3] bytes -> out_hwc [n][128][128][3] bytes and, when `images`
 *                                     is not NULL, images [n,3,128,128] fp32 in [-1,1] of the same bytes (the table of
 *                                     ndp_eval_frames_u8), in ONE launch.  tables: device copy of the built tables
 *                                     (table_bytes >= ndp_resize_workspace_bytes(H, W)); a table that was built for
 *                                     another size gives wrong pixels but no access outside the frames.
 *                                     rows_per_band: 0 (chosen from n), or 1, 2, 4, 8, 16 output rows per workgroup --
 *                                     the result does not depend on it.  All device pointers 4-byte aligned;
 *                                     1 <= n_images <= 65536.  Integer arithmetic, no atomics: bit-reproducible. */
int64_t ndp_resize_workspace_bytes(int64_t height, int64_t width);
int ndp_resize_build_tables(int64_t height, int64_t width, void *tables_host, int64_t bytes);
int ndp_resize_lanczos_u8(const uint8_t *frames_hwc, int64_t n_images, int64_t height, int64_t width, const void *tables,
                          int64_t table_bytes, int rows_per_band, uint8_t *out_hwc, float *images, void *stream);

/* -------------------------------------------------------- trajectory store ---
 * A directory of trajectory bundles (bundle.py) kept in device memory, and the assembly of a batch
 * from it (trajectory_store.py): B trajectory indices and a window of seq_length steps from seq_start become the packed
 * JPEG streams that ndp_jpeg_decode_u8 takes plus the matching rows of the float tables.
 *   blob           device bytes of all streams back to back, 4-byte aligned; blob_bytes is the size of the allocation:
 *                  nothing is read at or past blob + blob_bytes, or before blob
 *   frame_offsets  [n_traj * steps + 1] device int64, non-decreasing within 0..blob_bytes: frame t of trajectory i is
 *                  blob[frame_offsets[i * steps + t] .. frame_offsets[i * steps + t + 1])
 *   states / actions / goal   [n_traj][steps][25] / [n_traj][steps][4] / [n_traj][3] device floats
 *   indices        [batch] device int64.  An index outside 0..n_traj-1 gives that trajectory zero-length streams and all-zero
 *                  rows, sets NDP_STORE_BAD_INDEX in *status and causes no access outside the tables.  Duplicates are fine.
 *   out_buffer     device bytes, 16-byte aligned, `capacity` long (batch * seq_length * the longest stream always fits).
 *                  Stream s = b * seq_length + t of the batch is out_buffer[out_offsets[s] .. out_offsets[s+1]),
 *                  out_offsets[0] = 0: the bytes and the offsets that packing the same streams in the same order on the
 *                  host gives.  Nothing is written at or past out_offsets[batch * seq_length], nor at or past `capacity`
 *                  (a batch that does not fit sets NDP_STORE_CAPACITY; out_offsets are then still the full ones).
 *   out_offsets    [batch * seq_length + 1] device int64
 *   out_states / out_actions / out_goal   [batch][seq_length][25] / [batch][seq_length][4] / [batch][3] device floats, the
 *                  tables' bits
 *   status         one device int32, written by every call: 0 or an OR of NDP_STORE_*
 * n_traj * steps and batch * seq_length are at most 2^22; seq_start + seq_length <= steps.  Two launches, no host
 * synchronisation, no allocation, no atomics: two calls give the same bytes. */
#define NDP_STORE_BAD_INDEX 1
#define NDP_STORE_CAPACITY  2
int ndp_store_gather(const uint8_t *blob, int64_t blob_bytes, const int64_t *frame_offsets, const float *states,
                     const float *actions, const float *goal, int64_t n_traj, int steps, const int64_t *indices,
                     int64_t batch, int seq_start, int seq_length, uint8_t *out_buffer, int64_t capacity,
                     int64_t *out_offsets, float *out_states, float *out_actions, float *out_goal, int32_t *status,
                     void *stream);

/* ------------------------------------------- planner: cross-entropy refinement ---
 * One iteration of the cross-entropy method on a scored population of action sequences (evaluation.py: mpc_plan /
 * plan_step with `cem`), in ONE launch, one workgroup of 256 threads per trajectory.  A population is seq [Th][B][R][4]:
 * slice ts is the [B*R,4] action operand of ndp_fm_forward, no gather.
 *   err        [B,R] device: the population's scores (ndp_eval_score_select's err)
 *   seq_in     [Th,B,R,4] device: the population that was scored
 *   normal     [Th,B,R,4] device: standard normal draws (ndp_normal_noise); row 0 of every (ts, b) is not read
 *   first      1: mean / std / best_err are only written (no smoothing, no running minimum); 0: they are in/out
 *   low4/high4 host, 4 floats each: the bounds of the 4 action components
 *   mean, std  [B,Th,4] device; seq_out [Th,B,R,4] device; best_err [B] device; elite_idx [B,elites] device int32 or NULL
 * Ranking: row i comes before row j when e_i < e_j, or e_i == e_j and i < j; a NaN error comes after every number,
 * NaNs among themselves by index.  Rank 0 is the row ndp_eval_score_select picks without `forced` (whenever that
 * error is below its sentinel 1e10).  E' = min(elites, number of non-NaN errors); elite_idx[b] = the E' best rows in rank
 * order, then -1.
 * Refit, per component d of the D = 4 Th: the fp64 sum over the E' elites in rank order / E'; the fp64 sum of the
 * squared deviations from that mean / E' (population variance), fp64 sqrt; unless `first`, mean = momentum * mean_old +
 * (1 - momentum) * m and likewise std, in fp64, each product and sum rounded (no contraction); std = max(std, min_std);
 * each rounded to fp32 once.  E' == 0: mean and std stay (with `first`: 0 and min_std).
 * Resample: row 0 of seq_out is the rank-0 row of seq_in, bit for bit (E' == 0: row 0).  Every other element is
 * (float)((double)std * (double)n + (double)mean) -- the product is exact in fp64 --, clamped to [low, high] of its
 * component with fmaxf / fminf; a NaN stays NaN.
 * best_err[b] = min(best_err[b], e_rank0); a NaN never replaces a number (with `first`: e_rank0).
 * 1 <= B <= 65535, 2 <= R <= NDP_MAX_SAMPLES, 1 <= elites <= R, 1 <= Th <= 32, low <= high per component,
 * 0 <= momentum < 1, min_std >= 0; seq_in, normal and seq_out 16-byte aligned.  A limit exceeded, seq_out aliasing
 * seq_in or normal, a null required pointer: NDP_E_ARG, nothing launched.  No atomics, no scratch memory, no host
 * synchronisation: two calls give the same bits.  The caller owns every buffer.
 *
 * ndp_normal_noise: out[0 .. n) standard normal, Box-Muller over ndp_uniform_noise's stream: with U = the uniforms of
 * the same (seed, *offset_dev), pair j takes u1 = U[2j], u2 = U[2j+1], r = sqrtf(-2 logf(1 - u1)) (1 - u1 > 0: no
 * infinity), out[2j] = r cosf(2 pi u2), out[2j+1] = r sinf(2 pi u2) in fp32; an odd n drops the last sine. */
int ndp_plan_cem_update(const float *err, const float *seq_in, const float *normal, int64_t n_traj, int rollouts,
                        int steps, int elites, int first, float momentum, float min_std, const float *low4,
                        const float *high4, float *mean, float *std, float *seq_out, float *best_err,
                        int32_t *elite_idx, void *stream);
int ndp_normal_noise(float *out, int64_t n, uint64_t seed, const int32_t *offset_dev, void *stream);

/* ndp_plan_update: ndp_plan_cem_update with the weighting of the refit chosen and its one flag `first` split in two; the
 * same kernel body, every other argument, limit and refusal as above.  ndp_plan_cem_update is this call with weighting =
 * NDP_PLAN_ELITES and smooth = !first, and keeps its bits.
 *   smooth     1: the refit is smoothed against the mean / std it is given (in/out); 0: they are only written.  E' == 0:
 *              mean and std stay with smooth = 1, are 0 and min_std with smooth = 0
 *   first      1: best_err is only written; 0: it is the running minimum.  A planning step that starts from a carried
 *              prior (ndp_plan_warm) runs its first update with smooth = 1, first = 1
 *   weighting  NDP_PLAN_ELITES: the refit above.  NDP_PLAN_MPPI: ranking, E', elite_idx, row 0, best_err, resampling and
 *              clamping as above; the refit over the E' elites x_0 .. x_{E'-1} with errors e_0 <= e_1 <= ... in rank
 *              order weighs them, in fp64: w_0 = 1; w_k = 1 where e_k == e_0; otherwise w_k = exp(-((double)e_k -
 *              (double)e_0) / (double)temperature), so an infinite e_k weighs 0, and e_0 == inf gives all ones through
 *              the equality rule, never inf - inf.  W = sum w_k in rank order (W >= 1: no division by zero); m = sum w_k
 *              x_k / W; s = sqrt(sum w_k (x_k - m)^2 / W): fp64, fixed order, every product and sum rounded (no
 *              contraction), w_k (d d) with the square first; then the smoothing, the floor and the one rounding to fp32
 *              as above.  The weights are computed once per elite, not per component.
 *   temperature  with NDP_PLAN_MPPI finite and > 0, on the scale of err (ndp_eval_score_select: the pixel MSE of normalised
 *              images); not read with NDP_PLAN_ELITES
 * weighting, smooth or first outside their values, a bad temperature: NDP_E_ARG, nothing launched.
 *
 * ndp_plan_warm: the fit of one planning step turned into the prior and the injected rows of the next, in ONE launch.
 *   mean_prev, std_prev  [B,steps_prev,4] device: the previous planning step's fit
 *   normal     [steps,B,W,4] device: standard normal draws; row 0 of every (ts, b) is not read
 *   mean, std  [B,steps,4] device, written: with src(ts) = min(ts + 1, steps_prev - 1), mean[ts] = mean_prev[src(ts)] bit
 *              for bit and std[ts] = max(std_prev[src(ts)], warm_std); a NaN deviation gives warm_std
 *   warm       [steps,B,W,4] device, written: row 0 is mean[ts] clamped to [low, high] of its component (a NaN stays NaN),
 *              rows 1 .. W-1 are (float)((double)std * (double)n + (double)mean), clamped: ndp_plan_cem_update's draw
 * 1 <= B <= 65535, 1 <= W = rows <= NDP_MAX_SAMPLES - 1, 1 <= steps <= steps_prev <= 32, warm_std finite and >= 0, low <=
 * high per component, every buffer 16-byte aligned.  A limit exceeded, a null pointer, a misaligned buffer, an output
 * that is one of the inputs or another output: NDP_E_ARG, nothing launched.  One thread per row, 16-byte loads and
 * stores, no atomics, no scratch memory, no host synchronisation: two calls give the same bits. */
#define NDP_PLAN_ELITES 0
#define NDP_PLAN_MPPI   1
int ndp_plan_update(const float *err, const float *seq_in, const float *normal, int64_t n_traj, int rollouts, int steps,
                    int elites, int weighting, float temperature, int smooth, int first, float momentum, float min_std,
                    const float *low4, const float *high4, float *mean, float *std, float *seq_out, float *best_err,
                    int32_t *elite_idx, void *stream);
int ndp_plan_warm(const float *mean_prev, const float *std_prev, const float *normal, int64_t n_traj, int rows,
                  int steps_prev, int steps, float warm_std, const float *low4, const float *high4, float *mean,
                  float *std, float *warm, void *stream);

/* ------------------------------------------------ planner: gradient refinement ---
 * The gradient stage of one planning step (evaluation.py: `grad=GradSettings(...)`): after the
 * sampling rounds, the G best rows of the population are refined by J steps of gradient descent on the planner's own
 * score -- the MSE of the forward model's open-loop Th-step prediction against the goal image -- and written over the G
 * worst rows.  With R rows per trajectory, 1 <= G <= R / 2 (integer division), so the two sets are disjoint and the
 * originals stay in the population: the last selection can only gain.  Per iteration: Th eval-mode ndp_fm_forward passes
 * on the B * G rows, each on a workspace of its own, ndp_plan_goal_grad on the last predictions, ndp_fm_input_grads for
 * ts = Th-1 .. 0 (d_state_cur of pass ts is d_out of pass ts - 1; NULL at ts = 0; d_actions goes to grad[ts]), and
 * ndp_plan_grad_step.  Rows are independent: the seed is the gradient of the SUM of the rows' errors.
 *
 * ndp_plan_goal_grad: pred [n_rows,3,128,128], goal [n_goal,3,128,128]; row i is compared with goal row i /
 * rows_per_goal; (n_rows - 1) / rows_per_goal < n_goal.  ONE launch, one workgroup per row.
 *   err [n_rows]   the bits of ndp_eval_score_select's err on the same operands: with d = (double)pred - (double)goal
 *                  (exact for operands of like magnitude), "thread" t of 256 folds the row's elements t, t + 256, ... in
 *                  that order into s_t = fma(d, d, s_t) (ONE rounding per element, s_t = 0 at first); red = s; for w =
 *                  128, 64, .. 1: red[t] += red[t + w] for t < w; err = (float)(red[0] / 49152.0)
 *   d_pred [n_rows,3,128,128] = (pred - goal) * c with c = (float)(2.0 / 49152.0): one fp32 subtraction and one fp32
 *                  multiplication, the gradient of the row's err.  A NaN stays NaN
 * d_pred may be pred itself (in place) or disjoint from it; any other overlap, an output that overlaps goal, err inside
 * an image buffer, a null pointer, a misaligned image buffer (16 bytes), n_rows < 1, rows_per_goal < 1: NDP_E_ARG.  Loads
 * and stores are 16 bytes wide; no atomics, no scratch memory: two calls give the same bits.
 *
 * ndp_plan_grad_gather: err [B,R] and seq [Th,B,R,4] as in ndp_plan_cem_update, ranked by its order (NaN after every
 * number, ties and NaNs by index).  ONE launch, one workgroup per trajectory.
 *   src [B,G] int32   the rows of rank 0 .. G-1;   dst [B,G] int32   the rows of rank R-G .. R-1
 *   seq_g [Th,B,G,4]  row g = row src[b][g] of seq, bit for bit;   m, v [Th,B,G,4] = 0
 * 1 <= B <= 65535, 2 <= R <= NDP_MAX_SAMPLES, 1 <= G = rows <= R / 2, 1 <= Th <= 32; seq, seq_g, m, v 16-byte aligned and
 * pairwise disjoint, src != dst.
 *
 * ndp_plan_grad_step: update number t >= 1 of the rows seq_g [Th,B,G,4] (in/out) along grad [Th,B,G,4].  ONE launch, one
 * thread per row.  Every element in fp64 from the fp32 inputs (lr, beta1, beta2, eps are the fp32 arguments widened),
 * every product, sum, quotient and root rounded on its own (no contraction):
 *   NDP_PLAN_SGD   a' = a - lr * g
 *   NDP_PLAN_ADAM  m' = beta1 * m + (1 - beta1) * g;  v' = beta2 * v + (1 - beta2) * (g * g);
 *                  a' = a - (lr * (m' / c1)) / (sqrt(v' / c2) + eps),  c_i = 1 - p_i, p_i = beta_i multiplied t times onto
 *                  1.0 in fp64 (t roundings, no pow); m' and v' enter a' unrounded
 * a', m' and v' are rounded to fp32 once; a' is then clamped to [low, high] of its component (fmaxf / fminf, a NaN stays
 * NaN).  m, v [Th,B,G,4] in/out, read and written only by NDP_PLAN_ADAM (NULL allowed with NDP_PLAN_SGD).  A row with a
 * gradient component among its Th * 4 that is not finite is not moved, and its m and v stay.
 *   curve_out [B,G] or NULL   receives a copy of err_g [B,G] (required with curve_out): the rows' errors before the update
 *   dst [B,G] int32 and seq_full [Th,B,R,4], both or neither: row (b, g) of the result -- moved or not -- is also written
 *                  to row dst[b][g] of seq_full (an index outside 0..R-1: not written); every other row keeps its bits
 * 1 <= B <= 65535, 1 <= G = rows <= NDP_MAX_SAMPLES / 2, with seq_full 2 G <= R = rollouts <= NDP_MAX_SAMPLES, 1 <= Th <=
 * 32, 1 <= t <= 65535, lr finite and > 0, 0 <= beta < 1, eps finite and >= 0, low <= high per component; grad, seq_g, m, v,
 * seq_full 16-byte aligned and pairwise disjoint.
 * For all three: a limit exceeded, a null required pointer, a misaligned buffer, overlapping outputs: NDP_E_ARG, nothing
 * launched.  No atomics, no scratch memory, no host synchronisation: two calls give the same bits.  The caller owns
 * every buffer. */
#define NDP_PLAN_SGD  0
#define NDP_PLAN_ADAM 1
int ndp_plan_goal_grad(const float *pred, int64_t n_rows, const float *goal, int64_t n_goal, int rows_per_goal,
                       float *err, float *d_pred, void *stream);
int ndp_plan_grad_gather(const float *err, const float *seq, int64_t n_traj, int rollouts, int steps, int rows,
                         int32_t *src, int32_t *dst, float *seq_g, float *m, float *v, void *stream);
int ndp_plan_grad_step(const float *grad, float *seq_g, float *m, float *v, const float *err_g, int64_t n_traj, int rows,
                       int steps, int t, int optimizer, float lr, float beta1, float beta2, float eps,
                       const float *low4, const float *high4, float *curve_out, const int32_t *dst, float *seq_full,
                       int rollouts, void *stream);

/* --------------------------------------------------------------- push world ---
 * A small FetchPush-like world of the project's own (push_world.py): a gripper, a block and a goal
 * on a table, the reference's 4-component actions, n environments at once.  The world is in metres.
 *
 * State per environment: fp32 state[8] = gx, gy, gz, ox, oy, oz, tx, ty -- gripper xyz, object xyz, goal xy.  oz (0.425)
 * and the goal never change in a step. */
#define NDP_WORLD_X0        1.09     /* the table window: [X0, X0 + SIDE] x [Y0, Y0 + SIDE] */
#define NDP_WORLD_Y0        0.50
#define NDP_WORLD_SIDE      0.50
#define NDP_WORLD_REST_X    1.34     /* gripper rest position */
#define NDP_WORLD_REST_Y    0.75
#define NDP_WORLD_Z_MIN     0.42     /* gripper height range */
#define NDP_WORLD_Z_MAX     0.60
#define NDP_WORLD_Z_CONTACT 0.47     /* below this height the gripper touches the block */
#define NDP_WORLD_OBJECT_Z  0.425
#define NDP_WORLD_R_G       0.02     /* gripper radius */
#define NDP_WORLD_R_O       0.03     /* object radius */
#define NDP_WORLD_R         (NDP_WORLD_R_G + NDP_WORLD_R_O)   /* contact distance */
#define NDP_WORLD_STEP      0.05     /* move per step at full action */
#define NDP_WORLD_SUB       4        /* substeps per step */
#define NDP_WORLD_RING      0.008    /* width of the goal ring */
#define NDP_WORLD_SHADOW    0.6      /* shadow offset per metre of height above Z_MIN, in both axes */
/* Step.  All arithmetic is fp64 on the fp32 inputs, every operation rounded on its own (no contraction), the results
 * rounded to fp32 once at the end.  clamp(v, lo, hi) is v < lo ? lo : (v > hi ? hi : v).
 *     a_c = NaN -> 0;  m = STEP * clamp(a[0:3], -1, 1) / SUB         a[3] is ignored (FetchPush locks the fingers)
 *     SUB times:
 *         g = clamp(g + m) to [X0, X0+SIDE] x [Y0, Y0+SIDE] x [Z_MIN, Z_MAX]
 *         if g.z < Z_CONTACT:
 *             d = o.xy - g.xy;  r2 = d.x*d.x + d.y*d.y
 *             if r2 < R*R:
 *                 f = R / sqrt(r2);  o.xy = r2 > 0 ? (g.x + d.x*f, g.y + d.y*f) : (g.x + R, g.y)
 *                 clamp o.xy to [X0+R_O, X0+SIDE-R_O] x [Y0+R_O, Y0+SIDE-R_O]
 * A raised gripper passes over the block; a block pushed against the wall stays there and the gripper may overlap it; a
 * gripper that descends onto the block pushes it out sideways.
 *
 * Render.  Frames are S x S bytes HWC (row py, column px, RGB), S a multiple of 4, 32 <= S <= 1024.  One quantisation,
 * then integers: q(v) = llrint(v * (16 * S / SIDE)) in fp64, round-half-even, v * scale saturated to [-8192, 24576]
 * first (NaN: -8192) so that int32 holds every squared distance; the unit is a sixteenth of a pixel.  Centres are
 * (q(x - X0), q(y - Y0)); radii are q(radius).
 * Coverage: pixel (px, py) has 16 sample points (16 px + 2 + 4 i, 16 py + 2 + 4 j), i, j in 0..3.  A sample is inside a
 * disc iff dx^2 + dy^2 <= r^2, inside a ring iff rin^2 <= dx^2 + dy^2 <= rout^2; k = the samples inside, 0..16.
 * Blend, per channel and in this order, c = (c * (16 - k) + fg * k + 8) >> 4:
 *   1 table    (168, 160, 150), minus 12 on each channel where ((px / (S/8)) + (py / (S/8))) & 1 (integer divisions)
 *   2 goal     ring about t, rout = R_O, rin = R_O - RING, colour (40, 200, 60)
 *   3 shadow   disc R_G about (g.x + SHADOW * (g.z - Z_MIN), g.y + SHADOW * (g.z - Z_MIN)), fg = (c * 10 + 8) >> 4 of
 *              the colour under it
 *   4 object   disc R_O about o.xy, colour (20, 20, 235)
 *   5 gripper  disc of radius R_G * (1 + (g.z - Z_MIN) / (Z_MAX - Z_MIN)) about g.xy, colour (250, 245, 10)
 * Shapes at the window's edge are clipped by the frame.
 *
 *   ndp_world_step_render  state_in [n][8], actions [n][4] -> state_out [n][8] (not state_in) and, unless frames_hwc is
 *                          NULL, the frames [n][S][S][3] of the NEW state; one launch
 *   ndp_world_render       the frames of a given state; one launch
 * size as above, 1 <= n <= 65535, frames_hwc 4-byte aligned.  A bad size or n, a null required pointer, state_out ==
 * state_in: NDP_E_ARG, nothing launched.  No atomics, no scratch memory, no host synchronisation: two calls give the same
 * bits.  The caller owns every buffer. */
int ndp_world_step_render(const float *state_in, const float *actions, int64_t n, int size, float *state_out,
                          uint8_t *frames_hwc, void *stream);
int ndp_world_render(const float *state, int64_t n, int size, uint8_t *frames_hwc, void *stream);

/* ------------------------------------------------------------ measurement ---
 * Per-kernel timing for bench.py: while enabled (per host thread) every kernel
 * this library launches is bracketed by hipEvents recorded on the stream it is
 * launched on.  Must be off during graph capture.
 * ndp_timing_collect synchronises on the recorded events, sums the elapsed ms
 * per kernel name and resets the record: names receives "name0;name1;..."
 * (at most names_len bytes), total_ms / counts up to max_kernels entries.
 * Returns the number of distinct kernels; 0 with ndp_last_error() set on failure. */
int ndp_timing_enable(int on);
int ndp_timing_collect(char *names, int names_len, float *total_ms, int32_t *counts,
                       int max_kernels);

#ifdef __cplusplus
}
#endif
#endif /* NDP_H_ */
