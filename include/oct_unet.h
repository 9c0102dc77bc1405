/*
 * oct_unet.h -- C ABI of the MI355X-native OCT U-Net engine (liboct_unet_hip.so).
 *
 * This is the drop-in boundary for the ONE hot path of
 * NIH-NEI/oct-image-segmentation-models: the U-Net forward/backward + softmax/
 * Dice head that the reference delegates to tf.keras (Model.fit / Model.predict).
 * Plain C, plain pointers and sizes, no torch types.  Every device buffer is
 * owned by the CALLER (any allocator: torch, hipMalloc); the handle owns only
 * host-side plans.  No entry point allocates device memory, so every call after
 * oct_unet_create() is hipGraph-capturable.  All launches are asynchronous on
 * the caller-supplied stream.  One handle per GPU rank, driven by one host
 * thread.
 *
 * Reference interface each entry point replaces (paths relative to
 * /root/reference/oct_image_segmentation_models/):
 *
 *   oct_unet_create / _layer_info      UNet.__init__/build_model      models/unet.py:61-153
 *   params/state buffer layout         Model.get_weights/set_weights  training.py:319-342 (checkpoint, early stop)
 *   oct_unet_forward (training=0)      loaded_model.predict(...)      evaluation/evaluation.py:129-135,
 *                                                                     prediction/prediction.py:75-81
 *   oct_unet_forward (training=1)      Model.fit train step (fwd)     training/training.py:401-407
 *     x_is_u8 preprocessing            get_preprocess_input_fn x/255  models/unet.py:87-91
 *     io.argmax                        perform_argmax                 common/utils.py:80-112
 *   oct_boundary_maps_soft             perform_argmax(bin=False) -> convert_predictions_to_maps_semantic  common/utils.py:80-168
 *   oct_render_rgba                    save_image_plot / save_segmentation_plot (own line rule)  common/plotting.py:169-278
 *   oct_unet_loss_dice                 dice_loss_micro/_macro         common/custom_losses.py:47-81
 *                                      dice_coef_micro/_macro         common/custom_metrics.py:18-77
 *   oct_unet_set_bce_dice / _loss_bce_dice  bce_dice_loss             common/custom_losses.py:84-91
 *   oct_unet_backward                  Keras autodiff of the above    training/training.py:262-266,401-407
 *   oct_adam_step / oct_sgd_step       optimizer.apply_gradients      training/training.py:190-193
 *   oct_opt_step                       ... of any other opt_con, and the clipnorm / clipvalue / global_clipnorm options
 *   gradient buffer (caller-owned)     MirroredStrategy all-reduce    training/training.py:185-188,243
 *   oct_unet_graph_capture_infer / oct_unet_graph_launch  (none: replaces per-call Keras dispatch overhead, evaluation.py:108-135)
 *   oct_unet_infer, kind MC / oct_mc_update  (none: Monte-Carlo dropout prediction; the Dropout(0.5) it keeps on is models/unet.py:130)
 *   oct_unet_infer, kind TTA / oct_tta_update / oct_flip_batch  (none: test-time augmentation, the flips of flip_aug at prediction time)
 *   oct_augment_batch                  BatchGenerator.get_aug_fly/_nofly common/data_generator.py:140-283,
 *                                      flip_aug / add_noise_aug       common/augmentation.py:43-103
 *   oct_pad_batch / oct_crop_batch     (none: Keras raises on a size that is no multiple of 2^pool_layers, in the skip concatenation)
 *   oct_warp_batch                     (none at training time; the per-column np.roll of roll_image_offset /
 *                                      flatten_image_boundary        dataset_construction.py is its dataset-preparation kin)
 *   oct_elastic_batch                  (none: the smooth random elastic deformation of the U-Net paper, a training augmentation)
 *   oct_photo_batch                    (none: blur, column shadows and a gamma / brightness / contrast table, a training
 *                                      augmentation)
 *   oct_contrast_batch                 (none: CLAHE / percentile stretch of the uint8 scans in front of training, evaluation
 *                                      and prediction)
 *   oct_edge_weight_map / oct_unet_set_pixel_weights  (none: the border weight map of the U-Net paper / ReLayNet's boundary-
 *                                      weighted cross-entropy, as a per-pixel weight of the focal / BCE term)
 *   oct_calibration_counts / oct_temperature_apply / oct_temperature_nll  (none: reliability counts, ECE / NLL / Brier and
 *                                      temperature scaling of the softmax output, Guo et al. 2017)
 *   oct_ordered_decode                 (none: the best class map per column whose class index never decreases with depth)
 *   oct_components / oct_component_filter  (none: connected components of the class map, island removal, lesion counts)
 */
#ifndef OCT_UNET_H
#define OCT_UNET_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct oct_unet oct_unet;   /* opaque */
typedef void* oct_stream_t;         /* a hipStream_t (NULL = default stream) */

typedef struct oct_unet_cfg {
    int in_ch;            /* input_channels                       (unet.py:65)          */
    int n_cls;            /* num_classes, 2..16                   (training.py:176).  9..16 run   */
                          /*     the class-streaming head kernels (kernels_head_cls.hpp).  The   */
                          /*     probability maps are indexed with 32 bits downstream:           */
                          /*     max_batch*H*W*n_cls < 2^31 -- at 16 classes max_batch*H*W < 2^27 */
    int H, W;             /* image_height, image_width; multiples of 2^pool_layers     */
    int max_batch;        /* largest per-rank batch any call will pass                  */
    int start_neurons;    /* default 8; multiple of 4 in 4..64    (unet.py:69).  Widths  */
                          /*     above 32 run the channel-streaming head kernels ("head_wide"). */
                          /*     The 32-bit element index inside a layer bounds the size:      */
                          /*     max_batch*H*W*2*start_neurons < 2^31 -- at 64 channels         */
                          /*     max_batch*H*W*128 < 2^31, i.e. max_batch <= 127 at 256x512     */
    int pool_layers;      /* default 4                            (unet.py:70)          */
    int conv_layers;      /* default 2                            (unet.py:71)          */
    int enc_k;            /* 3  (enc_kernel (3,3))                (unet.py:72)          */
    int dec_k;            /* 2  (dec_kernel (2,2))                (unet.py:73)          */
    int dtype;            /* 0 = f32; 1 = bf16 activations / activation gradients (storage AND, */
                          /*     with mfma_mode 1, MFMA operands), f32 accumulation, f32 BN     */
                          /*     statistics, f32 parameters + gradients (BASELINE configs[2])   */
    int training;         /* 1: workspace also holds saved activations + gradients      */
    float bn_eps;         /* 1e-3  keras BatchNormalization default                     */
    float bn_momentum;    /* 0.99                                                       */
    float dropout_rate;   /* 0.5                                  (unet.py:130)         */
    int bn_unbiased_moving_var; /* 1: moving_var fed with Bessel-corrected batch var (TF fused BN) */
    unsigned long long seed;    /* dropout stream seed (differs per DP rank)            */
} oct_unet_cfg;

/* One Conv2D(+BN) node in Keras creation order; offsets are in floats. */
typedef struct oct_layer_info {
    char name[32];
    int kh, kw, cin, cout, has_bn;
    int out_h, out_w;
    size_t kernel_off, bias_off, gamma_off, beta_off;     /* into params / grads buffers */
    size_t moving_mean_off, moving_var_off;               /* into the state buffer        */
} oct_layer_info;

typedef struct oct_unet_io {
    float* probs;                 /* (B,H,W,n_cls) f32 softmax output, or NULL           */
    unsigned char* argmax;        /* (B,H,W) u8 class map, or NULL                       */
    const unsigned char* labels;  /* (B,H,W) u8 sparse labels, or NULL; enables Dice sums */
} oct_unet_io;

/* ---- sizing (host only, no GPU needed) ---- */
void   oct_unet_cfg_default(oct_unet_cfg* cfg);
int    oct_unet_cfg_check(const oct_unet_cfg* cfg);              /* 0 ok, <0 + oct_last_error() */
size_t oct_unet_param_count(const oct_unet_cfg* cfg);            /* trainable floats (487403 default, C=3) */
size_t oct_unet_state_count(const oct_unet_cfg* cfg);            /* BN moving stats (1712 default)         */
size_t oct_unet_workspace_bytes(const oct_unet_cfg* cfg);        /* activations, gradients, scratch        */
int    oct_unet_layer_count(const oct_unet_cfg* cfg);
int    oct_unet_layer_info(const oct_unet_cfg* cfg, int index, oct_layer_info* out);

/* ---- lifetime ---- */
/* params/grads: param_count floats; state: state_count floats; grads may be NULL when cfg.training==0. */
int  oct_unet_create(const oct_unet_cfg* cfg, float* params_dev, float* grads_dev, float* state_dev,
                     void* workspace_dev, size_t workspace_bytes, oct_unet** out);
void oct_unet_destroy(oct_unet* h);

/* ---- hot path ---- */
/* x: (B,H,W,in_ch) u8 (x_is_u8: /255 table applied on load) or f32 already in [0,1].
 * training=1: batch-statistic BN (+moving update), dropout, activations saved for backward. */
int oct_unet_forward(oct_unet* h, const void* x_dev, int x_is_u8, int B, int training,
                     const oct_unet_io* io, oct_stream_t stream);
/* After a forward with io.labels: out4_dev = {dice_loss_macro, dice_loss_micro,
 * dice_coef_macro, dice_coef_micro} (device floats). */
int oct_unet_loss_dice(oct_unet* h, float smooth, float* out4_dev, oct_stream_t stream);
/* focal_dice_loss (reference common/custom_losses.py:98-178, `SparseCategoricalFocalDiceLoss`):
 *   L = w * mean_px[ cw[y] * (1 - p_y)^gamma * (-log p_y) ] + (1 - w) * dice_loss_{macro|micro}
 * oct_unet_set_focal_dice selects it for the following forward / loss / backward calls (w = 0 restores the plain Dice
 * losses; class_weight_dev = n_cls device floats or NULL, caller-owned and kept alive).  oct_unet_loss_focal_dice is
 * oct_unet_loss_dice with 8 outputs: out8_dev = out4 + {focal term, w*focal + (1-w)*dice_macro,
 * w*focal + (1-w)*dice_micro, 0}; oct_unet_backward then differentiates the combination chosen by its `macro` flag. */
/* Unverifiable detail, isolated as a switch (like cfg.bn_unbiased_moving_var): third-party focal-loss==0.0.7 clips the
 * probabilities to [1e-7, 1-1e-7] for the logarithm; whether its (1 - p_y)^gamma modulation also sees the clipped value
 * cannot be checked here (package absent).  oct_set_option("focal_clip_modulation", 0) [default]: only the logarithm is
 * clipped; 1: both.  The two differ only where p_y is outside the clip range, by < 1e-7 relative in the loss and -- after
 * the softmax Jacobian, which multiplies by p_y -- by < 1e-6 of the gradient scale (tests/test_gpu_parity.py::
 * test_focal_clip_modulation_switch pins both against the oracle on a saturated head). */
int oct_unet_set_focal_dice(oct_unet* h, float focal_loss_weight, float gamma, const float* class_weight_dev);
int oct_unet_loss_focal_dice(oct_unet* h, float smooth, float* out8_dev, oct_stream_t stream);
/* bce_dice_loss (reference common/custom_losses.py:84-91): keras.losses.binary_crossentropy(y, p) + dice_loss_micro, i.e.
 *   L = (1 / (B H W C)) sum_{b,h,w,c} -( y ln(pc + e) + (1 - y) ln(qc + e) ) + dice_loss_micro
 * with p the softmax output, y the one-hot label, pc = clip(p, 1e-7, 1 - 1e-7), qc = clip(1 - p, 1e-7, 1 - 1e-7).  The
 * mean over B*H*W*C is Keras's mean over the class axis followed by SUM_OVER_BATCH_SIZE; under data-parallel training
 * oct_unet_backward's loss_scale carries the division by the number of replicas.  This restates Keras 2.9
 * (backend.binary_crossentropy, from_logits=False) from its definition: TensorFlow is not available to this project, so
 * parity with it is NOT pinned by a test (as for the focal loss); the tests compare with a torch-fp64 restatement.
 * oct_unet_set_bce_dice(h, 1) selects the loss for the following forward / loss / backward calls and clears a selected
 * focal_dice_loss; (h, 0), or oct_unet_set_focal_dice with weight > 0, clears it.  oct_unet_loss_bce_dice is
 * oct_unet_loss_dice with 8 outputs: out8_dev = out4 + {bce mean, 0, bce + dice_loss_micro, 0}.  oct_unet_backward
 * differentiates bce + dice_loss_micro (macro = 0); macro = 1 while the loss is selected is an argument error.
 * Unverifiable detail, isolated as a switch: whether the backend adds its epsilon once more inside the logarithms after
 * the clip.  oct_set_option("bce_inner_eps", 1) [default]: e = 1e-7; 0: e = 0.  Both are tested against the same
 * restatement under the same setting. */
int oct_unet_set_bce_dice(oct_unet* h, int on);
int oct_unet_loss_bce_dice(oct_unet* h, float smooth, float* out8_dev, oct_stream_t stream);
/* Ignore label: pixels whose label byte equals `label` do not count in the loss.  Per handle; holds for the following
 * forward / loss / backward calls (a forward made under another setting cannot be finalized or differentiated: call
 * forward again).  label = -1 [default] switches it off; n_classes..255 (n_classes up to 16) are accepted, anything else is an
 * argument error.
 * Without it a label byte >= n_classes is NOT ignored: such a pixel has an all-zero one-hot row and still counts in P, Ph
 * and the gradient.  With it, a pixel of that label
 *   - adds nothing to the Dice sums I, T, P, Ih, Ph of any class, nor to the focal / BCE sum; probs and argmax are
 *     written for it as for any pixel;
 *   - has dlogits = 0 exactly for every class (Dice, focal and BCE parts), so the gradient stored for the last conv block
 *     is 0 there and it adds nothing to the BN-backward statistics or the head's kernel / bias gradient;
 *   - and the focal mean divides by the number of COUNTED pixels of the batch, the BCE mean by that number times
 *     n_classes (the count is formed on the device by the loss call; oct_unet_backward reads it from the workspace).
 * Defined edge cases: an image without a counted pixel has per-class macro score s/s = 1 (smooth > 0); a batch without
 * one has focal = bce = 0, loss w*0 + (1-w)*0 for smooth > 0 and all-zero gradients; its dice_coef_micro is 0/0 = nan as
 * the reference's formula gives on empty sums, its dice_coef_macro 1 by that metric's own 1e-5 epsilon.
 * A captured graph (oct_unet_graph_capture_infer) keeps the setting it was captured under.
 * The reference has no counterpart; the tests compare with a torch-fp64 masked restatement. */
int oct_unet_set_ignore_label(oct_unet* h, int label);
/* Per-pixel weights of the pixel term.  weights_dev: (B,H,W) f32 of the NEXT batch (caller-owned, kept alive and refilled
 * in place between steps; e.g. oct_edge_weight_map's output), or NULL [default] = off.  With a map set, the focal term of a
 * counted pixel is w(x) cw[y] (1 - p_y)^gamma (-log p_y) and the BCE term of a counted pixel is w(x) sum_c(...), in the
 * forward sums and in oct_unet_backward alike; each term is multiplied by one float multiply, so a map of all 1.0f gives
 * the bits of the off path and a map of all 2.0f doubles the focal / BCE sum exactly.
 * NORMALISATION: the mean divides by what it divides by without a map -- B*H*W, or the counted pixels under an ignore
 * label -- as Keras's sample_weight does.  It does NOT divide by the sum of the weights.
 * The Dice term (plain or shaped), its five sums, the dice_coef metrics and the count of the ignore label never see the
 * map; with a plain Dice loss selected the map is accepted and has no effect.  Workspace sizes do not change.
 * Setting another pointer (or NULL) drops a pending forward's sums, as oct_unet_set_ignore_label does: call forward again
 * before the loss.  The same map must be in place for the forward and the backward of a step. */
int oct_unet_set_pixel_weights(oct_unet* h, const float* weights_dev);
/* Shape of the Dice term: Tversky weights, focal-Tversky exponent, class weights.  Per handle; holds for the following
 * forward / loss / backward calls; every call drops a pending Dice sum (call forward again).  s = NULL, or alpha = beta = 0.5,
 * gamma = 1, weight_mode = 0, is plain Dice: the launches and results are those of a handle that never had a shape.
 * All finalize arithmetic is fp64; s is the loss call's `smooth`.  For a triple of sums (I, T, P):
 *   N = 2I + s,  D = 2I + 2 alpha (P - I) + 2 beta (T - I) + s   [alpha = beta = 1/2: D = T + P + s],  u = 1 - N / D,
 *   L = u if gamma == 1, else max(u, 1e-7)^gamma (gradient 0 where the clamp is active).
 * macro: the triple is per (image b, class c) and loss = mean_b [ sum_c w_bc L_bc / sum_c w_bc ];
 * micro: I = sum_b sum_c w_c I_bc, likewise T and P, and there is one L.
 * weight_mode 0: every weight is 1.  1: w_bc = w_c = class_weight_dev[c], n_classes device floats, every entry finite and
 * >= 0 and not all zero; caller-owned, kept alive while the setting holds (read back once by this call to check it).
 * 2 ("volume", the generalized Dice loss): w = 1 / T^2 with T = T_bc of the image (macro) or T_c = sum_b T_bc of the batch
 * (micro); a class with T = 0 takes the largest weight among the classes with T > 0 of the same image / batch, and all
 * weights are 1 if there is none.  Weights depend on the labels only: constants of the differentiation.
 * Argument errors: alpha or beta < 0 or not finite, alpha + beta = 0, gamma outside (0, 8], weight_mode outside 0..2,
 * weight_mode 1 with a NULL or invalid array.
 * With a shape set the loss calls return the shaped macro / micro loss in outputs 0 and 1 and combine the focal or BCE term
 * with it in outputs 5 and 6; outputs 2 and 3 (dice_coef_macro / dice_coef_micro) are metrics and never change.  The
 * gradient for class c of a pixel with one-hot y is -m_c (y A_c - B_c) / D_c^2 with A = 2D - 2(1 - alpha - beta)N,
 * B = 2 alpha N, and m_c collecting the weight normalisation, gamma u^(gamma - 1) (0 under the clamp) and the macro / micro
 * scale; a class with m_c = 0 gets exactly 0.  The ignore label composes: ignored pixels never enter the sums.
 * The first call that sets a shape allocates the handle's table of backward constants on the device, O(max_batch * n_classes)
 * doubles, freed by the destroy call: the workspace keeps its size and a handle that never has a shape allocates nothing.
 * The reference has no counterpart; the tests compare with a numpy restatement and torch-fp64 autograd. */
typedef struct oct_dice_shape { float alpha, beta, gamma; int weight_mode; const float* class_weight_dev; } oct_dice_shape;
int oct_unet_set_dice_shape(oct_unet* h, const oct_dice_shape* s /* NULL: plain Dice */);
/* After training forward + loss_dice: fills the grads buffer with d(loss_scale*loss)/dparams. */
int oct_unet_backward(oct_unet* h, const unsigned char* labels_dev, int macro, float loss_scale,
                      oct_stream_t stream);

/* ---- data-parallel overlap (reference: tf.distribute.MirroredStrategy, training/training.py:185-188,243) ----
 * The gradient buffer has the parameter layout (Keras creation order: encoder, bottleneck, decoder, head) and backward
 * runs head -> decoder -> bottleneck -> encoder.  With a tail event set, oct_unet_backward sums the partial slabs of
 * every layer from the first bottleneck conv on as soon as that conv's gradients are queued and records the event behind
 * that sum (on the handle's internal side stream when "dw_side_stream" is on -- `stream` does not wait for it -- else on
 * `stream`): floats [oct_unet_grad_tail_offset(cfg), param_count) of grads are final from then on, so the launcher can
 * all-reduce that TAIL segment (bottleneck + decoder + head: 97 % of the floats) on a side stream (after
 * hipStreamWaitEvent) while the encoder backward still runs, and the remaining ENCODER segment [0, offset) after
 * backward.  hip_event: a hipEvent_t owned by the caller, NULL disables.  If oct_unet_backward returns an error the
 * event may not have been recorded and the handle's internal side stream has been joined to `stream` before returning. */
int    oct_unet_set_tail_event(oct_unet* h, void* hip_event);
size_t oct_unet_grad_tail_offset(const oct_unet_cfg* cfg);

/* ---- optimizers on flat buffers (Keras formulations) ---- */
int oct_adam_step(float* params_dev, const float* grads_dev, float* m_dev, float* v_dev, size_t n,
                  float lr, float beta1, float beta2, float eps, long step /*1-based*/, oct_stream_t stream);
int oct_sgd_step(float* params_dev, const float* grads_dev, float* momentum_buf_dev /*or NULL*/, size_t n,
                 float lr, float momentum, oct_stream_t stream);

/* ---- the Keras optimizer family with gradient clipping, on flat buffers (formulas: DESIGN.md section 13) ----
 * One streaming launch per step; clipping is applied on the fly and grads_dev is never written.  Stand-alone like the
 * two entry points above: no handle, no allocation, no host synchronisation, asynchronous on `stream`. */
enum { OCT_OPT_SGD = 0, OCT_OPT_ADAM = 1, OCT_OPT_ADAMAX = 2, OCT_OPT_RMSPROP = 3, OCT_OPT_ADAGRAD = 4, OCT_OPT_ADADELTA = 5 };
enum { OCT_OPT_NESTEROV = 1, OCT_OPT_AMSGRAD = 2, OCT_OPT_CENTERED = 4 };                 /* oct_opt_desc.flags */
enum { OCT_CLIP_NONE = 0, OCT_CLIP_VALUE = 1, OCT_CLIP_NORM = 2, OCT_CLIP_GLOBAL_NORM = 3 };  /* oct_opt_desc.clip_mode */

typedef struct oct_opt_desc {
    int kind;             /* OCT_OPT_*                                                                            */
    int flags;            /* OCT_OPT_NESTEROV (SGD with momentum), OCT_OPT_AMSGRAD (Adam), OCT_OPT_CENTERED (RMSprop) */
    int clip_mode;        /* OCT_CLIP_*: at most one kind of clipping per step                                     */
    float clip;           /* its threshold: > 0 for the norm modes, >= 0 for OCT_CLIP_VALUE                        */
    float lr;             /* learning rate of THIS step (decay / schedule already applied by the caller)          */
    float beta1, beta2;   /* Adam, Adamax                                                                          */
    float rho;            /* RMSprop, Adadelta                                                                     */
    float momentum;       /* SGD, RMSprop (0 = none)                                                               */
    float eps;            /* all but SGD                                                                           */
} oct_opt_desc;

/* State buffers of n floats each the optimizer needs (0..3), in the order the step takes them, or -1 for a bad descriptor:
 *   SGD       momentum != 0: [v]                           Adam      [m, v] (+ [vhat] with OCT_OPT_AMSGRAD)
 *   Adamax    [m, u]                                       RMSprop   [rms] (+ [mom] if momentum != 0) (+ [mg] if OCT_OPT_CENTERED)
 *   Adagrad   [a]  (the caller fills it with initial_accumulator_value)      Adadelta  [a, b]
 * Every other buffer starts at zero. */
int oct_opt_slot_count(const oct_opt_desc* desc);

/* Bytes of scratch a clipped step over n floats in n_vars variables needs (norm partials in double + one scale per variable). */
size_t oct_opt_scratch_bytes(size_t n_vars, size_t n);

/* One optimizer step (`step` is 1-based).  slots: HOST array of 3 device pointers, the state buffers above in that order
 * (entries past the slot count are ignored).
 * var_off_dev: the variable table for OCT_CLIP_NORM -- n_vars + 1 ascending offsets ON THE DEVICE, variable k being
 * [var_off[k], var_off[k+1]), var_off[0] = 0 and var_off[n_vars] = n (the pieces oct_unet_layer_info describes: kernel,
 * bias, gamma, beta of each conv); unused (may be NULL) in the other modes.  scratch_dev: oct_opt_scratch_bytes() bytes,
 * 16-byte aligned, for the two norm modes (else may be NULL).  The norm modes add two launches: per-variable partial sums of
 * squares in a fixed order, then their sum in double and scale = clip / max(norm, clip) -- no atomics, no host read. */
int oct_opt_step(const oct_opt_desc* desc, float* params_dev, const float* grads_dev, float* const* slots, size_t n,
                 long step, const unsigned long long* var_off_dev, size_t n_vars, void* scratch_dev, oct_stream_t stream);

/* ---- dropout stream control (parity tests replay the mask) ---- */
int oct_unet_set_dropout_step(oct_unet* h, unsigned long long step);
/* keep-mask (B, H/2^P, W/2^P, start_neurons*2^P) u8 {0,1} that a training forward at the current step uses */
int oct_unet_dropout_mask(oct_unet* h, int B, unsigned char* mask_dev, oct_stream_t stream);

/* ---- per-launch profiler: HIP events recorded around every kernel launch, on the launch stream ----
 * begin() arms it; every forward/backward call of this handle made on the calling thread is then recorded;
 * end() synchronises the device and returns one entry per (kernel instantiation, layer) with the summed
 * duration and the ALGORITHMIC flops/bytes of those launches (cost model). */
typedef struct oct_profile_entry {
    char kernel[80];
    char layer[32];
    int launches;
    double total_ms, flops, bytes;
} oct_profile_entry;
int oct_unet_profile_begin(oct_unet* h);
int oct_unet_profile_end(oct_unet* h, oct_profile_entry* out, int max_entries, int* n_out);

/* ---- post-step on device: (B,H,W) u8 class maps -> (B, n_cls-1, H, W) u8 boundary maps, exactly
 * convert_predictions_to_maps_semantic(one_hot(argmax)) of the reference (common/utils.py:115-168) ---- */
int oct_boundary_maps(const unsigned char* labels_dev, int B, int H, int W, int n_cls, int bg_ilm, int bg_csi,
                      unsigned char* maps_dev, oct_stream_t stream);

/* ---- soft boundary maps on device: (B,H,W,n_cls) f32 class probabilities -> (B, n_cls-1, H, W) u8 boundary maps, exactly
 * convert_predictions_to_maps_semantic of the probabilities themselves, which is what perform_argmax(bin=False) hands it
 * (common/utils.py:80-168); oct_boundary_maps is the same function of the arg-max's one-hot.  Restated in numpy, element
 * by element, by common/utils.py::soft_boundary_maps_reference.  For map m in 1..n_cls-1:
 *   flip = (m == 1 && bg_ilm) || (m == n_cls-1 && bg_csi);  k = flip ? m-1 : m;  f[r] = probability of class k in the
 *   pixel's column at row r.  In fp32, one IEEE operation per step:
 *     d[r] = 0 if H == 1;  f[1] - f[0] at r == 0;  f[H-1] - f[H-2] at r == H-1;  (f[r+1] - f[r-1]) / 2 otherwise
 *     (np.gradient along the rows);  d = -d if flip;  g[r] = 2 * max(d[r], 0);
 *     v = max(g[r] - g[(r+1) mod H], 0)        (the roll wraps: the last row subtracts row 0's g);
 *     out = (unsigned char)((int)(v * 255.0f) & 255)   (numpy's float32 -> uint8 cast: truncate, then wrap -- the rule
 *     oct_boundary_maps follows for 510 -> 254; with probabilities in [0,1] only rows 0 and H-1 can exceed 255).
 *   All steps but the two subtractions and the product with 255 are exact, and none is contracted with another, so the
 *   result equals numpy's bit for bit.
 * The inputs are finite floats, and the values are defined for [0,1], what the softmax delivers: NaN and infinity are
 * outside the contract (no fault, unspecified bytes).  Stand-alone like oct_boundary_maps: no handle, no allocation, one
 * asynchronous launch on `stream`, never waits, records into a stream capture.  probs_dev needs only its natural 4-byte
 * alignment, maps_dev none.  Errors (negative, oct_last_error(), nothing launched): null pointers, non-positive sizes,
 * n_cls outside 2..32, an output range overlapping the input. */
int oct_boundary_maps_soft(const float* probs_dev /* (B,H,W,n_cls) f32, the layout of oct_unet_io.probs */,
                           int B, int H, int W, int n_cls, int bg_ilm, int bg_csi,
                           unsigned char* maps_dev /* (B, n_cls-1, H, W) */, oct_stream_t stream);

/* ---- Monte-Carlo dropout on device (Gal & Ghahramani 2016; the reference has no counterpart: its Dropout(0.5) on the
 * bottleneck, models/unet.py:130, is only active in Model.fit).  T stochastic softmax outputs p^(0..T-1) of one batch are
 * folded, one call per sample, into running sums in a caller-owned workspace; the call for the last sample turns the sums
 * into the maps of oct_mc_out.  Restated in numpy, step by step, by common/utils.py::mc_reduce_reference.  All arithmetic is
 * fp32, one IEEE operation per step, none contracted with another:
 *   plogp(p) = p > 0 ? p * logf(p) : 0                 (logf: the OCML library function, not the fast intrinsic)
 *   h_t = -(plogp(p_0) + plogp(p_1) + ... )            (summed in class order) -- the entropy of sample t
 *   workspace: S_c (B,H,W,n_cls) then E (B,H,W).  t == 0: S_c = p_c, E = h_0 (no memset needed);  t > 0: S_c += p_c, E += h_t
 *   t == T-1:  m_c = S_c * float(1.0f / T)                                     -> mean_probs
 *              argmax = the lowest index among equal maxima of m                -> argmax
 *              entropy = -(plogp(m_0) + plogp(m_1) + ...)  (class order)         -> entropy      (predictive entropy, nats)
 *              mutual_info = max(entropy - E * float(1.0f / T), 0)              -> mutual_info  (BALD)
 *   mean_probs and argmax therefore equal the numpy restatement bit for bit; entropy and mutual_info agree with it to
 *   the accuracy of logf (about 1 ulp per term; 2e-5 absolute against fp64 for n_cls <= 32, T <= 64).
 * Calls are made with t in order 0..T-1 on one stream.  The call of the last sample does not write the sums back: the
 * workspace contents are unspecified afterwards.  Inputs are probabilities: finite, in [0,1] (NaN: no fault, unspecified
 * values).  Stand-alone like oct_boundary_maps_soft: no handle, no allocation, ONE asynchronous launch per call on `stream`
 * (grid-stride over pixels, no atomics, deterministic), never waits, records into a stream capture.  Pointers need their
 * natural alignment only; with 16-byte aligned buffers, n_cls <= 8 and B*H*W*n_cls % 4 == 0 the kernel moves float4s.
 * Errors (negative, oct_last_error(), nothing launched): null probs / workspace, null `out` when t == T-1, non-positive
 * sizes, n_cls outside 2..32, B*H*W >= 2^31, T outside 1..64, t outside 0..T-1, a workspace smaller than
 * oct_mc_workspace_bytes, output ranges that overlap the input, the workspace or each other. */
typedef struct oct_mc_out {
    float* mean_probs;            /* (B,H,W,n_cls) f32, or NULL */
    unsigned char* argmax;        /* (B,H,W) u8,        or NULL */
    float* entropy;               /* (B,H,W) f32,       or NULL */
    float* mutual_info;           /* (B,H,W) f32,       or NULL */
} oct_mc_out;
size_t oct_mc_workspace_bytes(int B, int H, int W, int n_cls);   /* B*H*W*(n_cls+1) floats; 0 = unsupported shape */
int oct_mc_update(const float* probs_dev /* (B,H,W,n_cls) f32 */, int B, int H, int W, int n_cls, int t, int T,
                  void* ws_dev, size_t ws_bytes, const oct_mc_out* out /* read when t == T-1 */, oct_stream_t stream);

/* ---- test-time augmentation on device: the softmax outputs of mirrored views of a batch, mirrored back and averaged ----
 * A view code v is in 0..3: bit 0 mirrors columns (xv = W-1-x, "flip_lr"), bit 1 mirrors rows (yv = H-1-y, "flip_ud");
 * 0 identity, 1 flip_lr, 2 flip_ud, 3 flip_both.  A flip is its own inverse.
 *
 * oct_flip_batch: dst[b, y, x] = src[b, yv, xv] over (B,H,W) pixels of `pixel_bytes` bytes each, the set oct_crop_batch
 * accepts (1, 2, 4, 8, 12, ..., 32: uint8 scans of 1 / 2 / 4 / ... channels, float32 scans of up to 8, every map of
 * oct_mc_out); the kernel only moves bytes.  Out of place.  Where a row is a whole number of dwords and both bases are
 * 4-byte aligned it moves dwords (pixels below 4 bytes: whole dwords from the mirrored position, their pixels reversed),
 * otherwise single bytes; no alignment is required.  common/utils.py::flip_reference restates it.
 * Errors (negative, oct_last_error(), nothing launched): null or overlapping buffers; non-positive B, H, W; pixel_bytes
 * outside the set; view outside 0..3; element counts that overflow the kernel's indexing (as oct_crop_batch).
 *
 * oct_tta_update is oct_mc_update with ONE change: the running sums and the outputs of pixel (b, y, x) take sample t's pixel
 * (b, yv, xv) under `view` -- sample t being the softmax output of the batch flipped by `view`, this mirrors it back while
 * folding.  Workspace (oct_mc_workspace_bytes), oct_mc_out, the fp32 operations, their order and the no-contraction rule
 * are oct_mc_update's: t == 0 assigns, t == T-1 finishes in registers, sums in class order, the arg-max the lowest index
 * among equal maxima.  common/utils.py::tta_reduce_reference restates it.  Hence
 *   - with view == 0 the four maps equal oct_mc_update's byte for byte;
 *   - for any view, folding the flipped sample (oct_flip_batch(p_t, view)) under that view equals oct_mc_update on p_t
 *     byte for byte.
 * With 16-byte aligned buffers, n_cls <= 8 and W % 4 == 0 the kernel moves float4s: 4 adjacent output pixels read 4 adjacent
 * source pixels, permuted in registers; every other case goes pixel by pixel.  One thread owns an output pixel: no
 * atomics, deterministic.  Stand-alone like oct_mc_update: no handle, no allocation, ONE asynchronous launch, never waits,
 * records into a stream capture.  Errors: those of oct_mc_update, and view outside 0..3, T outside 1..4. */
int oct_flip_batch(const void* src_dev, int B, int H, int W, int pixel_bytes, int view, void* dst_dev, oct_stream_t stream);
int oct_tta_update(const float* probs_dev /* (B,H,W,n_cls) f32 */, int B, int H, int W, int n_cls, int view, int t, int T,
                   void* ws_dev, size_t ws_bytes, const oct_mc_out* out /* read when t == T-1 */, oct_stream_t stream);

/* ---- inference: one chain of launches, described by oct_infer ----
 * Three independent choices:
 *   kind       OCT_INFER_PLAIN  one forward (training = 0).  The head writes out.mean_probs (its probabilities) and out.argmax
 *                               itself: no scratch, no reduction launch; out.entropy and out.mutual_info must be NULL.
 *              OCT_INFER_MC     Monte-Carlo dropout: the encoder and the bottleneck sit in front of the dropout and are
 *                               deterministic, so layers [0, k) run ONCE -- k = the up-convolution behind the bottleneck -- and
 *                               for t = 0..T-1 layers [k, head] run with the dropout stream of step step0 + t on the input of
 *                               layer k: exactly the keep-mask oct_unet_dropout_mask returns after oct_unet_set_dropout_step(
 *                               step0 + t), kept values scaled by 1 / (1 - dropout_rate) as in training.  The head writes
 *                               sample t to probs_scratch_dev and oct_mc_update(t, T) folds it into ws_dev.  T in 1..64.  With
 *                               dropout_rate == 0 the samples are identical.
 *              OCT_INFER_TTA    for t = 0..T-1: oct_flip_batch(input, views[t]) into x_view_dev (skipped for view 0: the forward
 *                               reads the input itself), a plain forward of it into probs_scratch_dev, oct_tta_update(views[t], t,
 *                               T) into ws_dev.  T in 1..4, views in 0..3.  x_view_dev: a batch like the input (same type, the
 *                               handle's size); may be NULL if every view is 0.  Each forward's probabilities are bit for bit
 *                               those of oct_unet_forward on the flipped batch.
 *              For MC and TTA `out` receives the maps of the T samples / of the mean prediction, ws_bytes >=
 *              oct_mc_workspace_bytes(B, cfg.H, cfg.W, n_cls), and at least one map is asked for.
 *   padding    x_pad_dev == NULL: x_dev is (B,cfg.H,cfg.W,in_ch); (H, W) must be the handle's size; out_crop is not read.
 *              x_pad_dev != NULL: x_dev is (B,H,W,in_ch), a size that is no multiple of 2^pool_layers, around a handle built at
 *              the padded size: oct_pad_batch of x_dev into x_pad_dev (B,cfg.H,cfg.W,in_ch) at (top, left) in front, the chain on
 *              x_pad_dev into `out` (padded-size buffers), and one oct_crop_batch per map that out_crop asks for, (B,H,W[,n_cls]);
 *              `out` must hold it.  The padded batch is THE input: the views are flips of the padded batch, the fold runs at the
 *              padded size and the crop comes last, so the result equals the unpadded chain of that handle on the padded batch,
 *              cropped.
 *   execution  oct_unet_infer runs the chain on `stream`; oct_unet_graph_capture_infer records the same launches into the
 *              handle's graph (replacing an earlier one) for oct_unet_graph_launch to replay -- one stream, no forked branch;
 *              it needs a non-default stream.  An MC chain is NOT captured (refused): the dropout step travels by value in
 *              the kernel arguments, so a replay would repeat the captured steps -- which is also why each call is cheap to vary.
 * Every kind prepares the weights once, runs BN from the moving statistics, works on training and inference handles, f32 and
 * bf16 (cfg.dtype 1), allocates nothing and is asynchronous.  No statistic rows are written, parameters, moving statistics
 * and the dropout step are as before the call, nothing is saved for a backward.  MC and TTA drop a pending Dice sum (a following
 * oct_unet_loss_dice needs a new oct_unet_forward with io.labels); PLAIN leaves the handle as oct_unet_forward(training = 0)
 * without labels does.  oct_unet_forward stays the training and labelled forward.
 * Errors (negative, oct_last_error(), nothing launched): null handle, descriptor or input; a kind outside the three; B outside
 * 1..max_batch; a size other than the handle's without x_pad_dev; PLAIN with entropy or mutual_info; MC / TTA: null scratch or
 * workspace, no map asked for, T out of range, a view outside 0..3, a flipped view without x_view_dev or with an input pixel
 * that oct_flip_batch does not take (in_ch * element size outside its set), the errors of oct_flip_batch, oct_mc_update and
 * oct_tta_update (workspace too small, overlapping ranges, ...); padded: the errors of oct_pad_batch, out_crop asking for a map
 * that `out` does not hold or that overlaps it; capture: also a default stream. */
enum { OCT_INFER_PLAIN = 0, OCT_INFER_MC = 1, OCT_INFER_TTA = 2 };
typedef struct oct_infer {
    const void* x_dev;            /* the batch, u8 (x_is_u8) or f32 in [0,1]                          */
    int x_is_u8, B;
    int kind, T;                  /* OCT_INFER_*; samples (MC) or views (TTA), ignored for PLAIN     */
    unsigned long long step0;     /* MC: dropout step of sample 0                                     */
    int views[4];                 /* TTA: T view codes                                                */
    void* x_view_dev;             /* TTA scratch: the flipped input                                   */
    float* probs_scratch_dev;     /* MC / TTA scratch: (B,cfg.H,cfg.W,n_cls) f32, one sample          */
    void* ws_dev; size_t ws_bytes;   /* MC / TTA: the reduction workspace                             */
    int H, W, top, left;          /* size of x_dev and its place inside the handle's size            */
    int pad_mode; float pad_value;   /* OCT_PAD_*, as oct_pad_batch (declared below)                  */
    void* x_pad_dev;              /* NULL: no padding                                                 */
    oct_mc_out out, out_crop;     /* maps at the handle's size; at (H, W), read only when padding    */
} oct_infer;
int oct_unet_infer(oct_unet* h, const oct_infer* d, oct_stream_t stream);
int oct_unet_graph_capture_infer(oct_unet* h, const oct_infer* d, oct_stream_t stream);
int oct_unet_graph_launch(oct_unet* h, oct_stream_t stream);

/* ---- evaluation metrics on device: average surface distance and robust Hausdorff distance of every foreground class
 * (reference evaluation/evaluation.py:207-262 -> common/custom_metrics.py:103-119 -> google-deepmind/surface-distance
 * compute_surface_distances / compute_average_surface_distance / compute_robust_hausdorff, 2D; results stored at
 * evaluation.py:573-597 and averaged at :783-803, :870-882).  A restatement of the un-vendored package: PARITY UNPINNED.
 * pred_dev, gt_dev: (B,H,W) u8 class maps; class c in 1..n_cls-1 is the mask (map == c).  Per (b, c) the 2x2-cell border
 * elements of both masks, their contour lengths, the exact Euclidean distance (spacing_row, spacing_col: physical size of
 * a pixel) of each to the nearest border element of the other mask, then out_dev (B, n_cls-1, 6) doubles:
 *   {asd_gt_to_pred, asd_pred_to_gt, perc_gt_to_pred, perc_pred_to_gt, n_surfels_gt, n_surfels_pred}
 * asd = length-weighted mean distance (NaN without border elements, +inf when the other mask has none); perc = the
 * length-weighted `percent` percentile (+inf without border elements).  Hausdorff = max(perc_gt_to_pred, perc_pred_to_gt).
 * Deterministic (fixed-order sums, integer-count selection).  workspace_dev: oct_surface_workspace_bytes(B, H, W, n_cls)
 * bytes (0 = unsupported shape), caller-owned.  Rejected with an error: labels >= n_cls (checked on the device; the call
 * then waits for `stream` once), percent outside [0, 100], non-positive spacings, a workspace that is too small. */
size_t oct_surface_workspace_bytes(int B, int H, int W, int n_cls);
int oct_surface_distances(const unsigned char* pred_dev, const unsigned char* gt_dev, int B, int H, int W, int n_cls,
                          double spacing_row, double spacing_col, double percent,
                          void* workspace_dev, size_t workspace_bytes, double* out_dev, oct_stream_t stream);
/* oct_surface_distances_masked: the same metrics on partially labelled ground truth (host
 * restatement: common/custom_metrics.py::compute_surface_distances(..., valid=)).  A ground-truth pixel equal to
 * ignore_label (a value in n_cls..255) is unknown: a 2x2 cell is a border element only if none of its in-image pixels is
 * unknown, in the ground-truth mask and in the prediction mask alike (the validity comes from gt_dev for both; the zero
 * padding outside the image is known background).  Surfaces are those seen entirely inside the labelled region; the rim
 * of an unknown region is never one.  Only the column pass differs: workspace, output rows, distances, lengths, the
 * percentile and the NaN / +inf / 0 of an empty element set are those of oct_surface_distances, and with no pixel equal
 * to ignore_label the rows are equal bit for bit.  Rejected as there; the label check passes ignore_label in gt_dev only
 * (any other value >= n_cls there, and every value >= n_cls in pred_dev, is an error), and ignore_label outside
 * n_cls..255 is an argument error. */
int oct_surface_distances_masked(const unsigned char* pred_dev, const unsigned char* gt_dev, int B, int H, int W, int n_cls,
                                 int ignore_label, double spacing_row, double spacing_col, double percent,
                                 void* workspace_dev, size_t workspace_bytes, double* out_dev, oct_stream_t stream);

/* ---- training augmentations on device: (B,H,W,C) u8 images -> f32 in [0,1], flipped or with noise added; (B,H,W) u8 labels
 * flipped alongside (reference common/data_generator.py:140-283 chooses an augmentation per sample, common/augmentation.py:
 * 43-103 applies it; its noise is skimage.util.random_noise, whose RNG stream is unpinned: the stream here is the library's
 * own, defined below and restated in numpy by common/augmentation.py device_aug_reference).  Stand-alone: no handle, no
 * allocation, one asynchronous launch on `stream`, graph-capturable.  Per sample b, op = ops_dev[b]:
 *   img = float32(x / 255.0), the u8 input definition of oct_unet_forward.
 *   kind 0 none, 1 flip up-down, 2 flip left-right: out = img at the (mirrored) position, labels mirrored the same way.
 *   Every other kind copies the labels.  A kind outside 0..5 is only visible on the device and is TREATED AS 0 (no
 *   device-side flag, no stream wait: validate before upload).  labels_dev == NULL or labels_out_dev == NULL: no labels written.
 *   Random words: Philox4x32-10 (Salmon et al., SC'11 / Random123), key = (seed low, seed high), counter =
 *   (e >> 1, 0, noise_id low, noise_id high) with e = (y*W + x)*C + c the element's index inside its sample (output
 *   position); element e owns words w0 = out[2(e&1)], w1 = out[2(e&1)+1].  Nothing depends on b, B or the launch geometry.
 *   u1 = ((w0 >> 8) + 1) 2^-24 in (0,1], u2 = (w1 >> 8) 2^-24 in [0,1); z = sqrt(-2 ln u1) cos(2 pi u2) (fp32).
 *   kind 3 gaussian: out = clip(img + (p0 + p1 z), 0, 1); kind 4 speckle: out = clip(img + img (p0 + p1 z), 0, 1);
 *     p0 = mean, p1 = sigma = sqrt(variance).
 *   kind 5 salt-and-pepper: flipped = ((w1 >> 8) 2^-24 <= p0), salted = ((w0 >> 8) 2^-24 <= p1); out = flipped ?
 *     (salted ? 1 : 0) : img; p0 = amount, p1 = salt_vs_pepper ("salt" = 1, "pepper" = 0).
 * Errors (negative, nothing launched): null x_u8_dev / ops_dev / x_out_dev, non-positive sizes, B > 65535 or
 * H*W*C >= 2^31, labels_out_dev without labels_dev, an output range overlapping an input range or the other output. */
typedef struct oct_aug_op {      /* one per sample of the batch, 32 bytes, in DEVICE memory */
    int   kind;
    float p0, p1, p2;
    unsigned long long noise_id; /* selects the sample's random stream */
    unsigned long long reserved;
} oct_aug_op;
int oct_augment_batch(const unsigned char* x_u8_dev, const unsigned char* labels_dev, const oct_aug_op* ops_dev,
                      int B, int H, int W, int C, unsigned long long seed,
                      float* x_out_dev, unsigned char* labels_out_dev, oct_stream_t stream);

/* ---- geometric training augmentations on device: (B,H,W,C) u8 images -> u8 images, each sample shifted per column or mapped
 * through an affine transform; (B,H,W) u8 labels moved alongside.  Runs in FRONT of oct_augment_batch, whose flips and noise
 * then apply to its output.  (The reference has only the per-column np.roll of roll_image_offset / flatten_image_boundary in
 * dataset_construction.py, as dataset preparation.)  Integer arithmetic only, so the kernel, the numpy restatement
 * (common/augmentation.py warp_reference) and the host augmentation path give the same bytes.  Stand-alone: no handle, no
 * allocation, one asynchronous launch on `stream`, graph-capturable.  Per sample b, op = ops_dev[b]; `/` below is FLOOR
 * division, `>>` an arithmetic shift, all intermediates are 64-bit signed integers.
 *   border, applied to every source index i of an axis of length n on its own:
 *     0 replicate: min(max(i, 0), n-1);  1 wrap: i mod n, non-negative;  2 constant: i outside 0..n-1 makes the tap read
 *     `fill` (image, low 8 bits) or `fill_label` (labels, low 8 bits).
 *   kind 0 none: copy.
 *   kind 1 column shift, a = p[0], b = p[1], c = p[2] in 1/256 pixel (translation, rise of the right edge against the centre,
 *     sag of both edges).  With t = 2x - (W-1), D = max(W-1, 1):
 *       s(x) = (a D^2 + b t D + c t^2 + 128 D^2) / (256 D^2)
 *       out[y, x, :] = in[src(y - s(x)), x, :], labels the same.  b = c = 0, a = 256 k, wrap: np.roll(image, k, axis=0).
 *   kind 2 affine, an inverse map: m00, m01, m10, m11 = p[0..3] in Q16, t0, t1 = p[4], p[5] in Q16 HALF pixels.  With
 *     X = 2x - (W-1), Y = 2y - (H-1):  U = m00 X + m01 Y + t0,  V = m10 X + m11 Y + t1,
 *       sx = (U + (W-1) 65536) >> 1,  sy = (V + (H-1) 65536) >> 1                       (source position in Q16 pixels)
 *     image: ix = sx >> 16, fx = (sx >> 8) & 255, iy, fy likewise; taps p00 = (ix, iy), p01 = (ix+1, iy), p10 = (ix, iy+1),
 *       p11 = (ix+1, iy+1), each through the border rule;
 *       out = ((256-fx)(256-fy) p00 + fx (256-fy) p01 + (256-fx) fy p10 + fx fy p11 + 32768) >> 16
 *     labels: the nearest pixel ((sx + 32768) >> 16, (sy + 32768) >> 16) through the border rule.
 *     m00 = m11 = 65536, rest 0 is the identity, byte for byte; m00 = m11 = -65536 flips both axes.
 *   Parameter ranges (OCT_WARP_MAX_*): H, W <= 16384, |a|, |b|, |c| <= 2^22, |m..| <= 2^20, t0, t1 any int32.  Then
 *     |a D^2 + b t D + c t^2 + 128 D^2| < 2^52 and |U|, |V| < 2^36: no intermediate leaves int64, and every source index
 *     fits an int32.  The ranges are only visible on the device: REFUSE anything outside them on the host, before upload
 *     (common/augmentation.py check_warp_ops).  A kind or border outside 0..2 is TREATED AS kind 0 (no device-side flag).
 *   labels_dev == NULL or labels_out_dev == NULL: no labels written.  Nothing depends on b, B or the launch geometry.
 * Errors (negative, nothing launched): null x_u8_dev / ops_dev / x_out_dev, non-positive sizes, B > 65535, H or W >
 * 16384, H*W*C >= 2^31, labels_out_dev without labels_dev, an output range overlapping an input range or the other output
 * (the stage gathers: it cannot run in place). */
#define OCT_WARP_MAX_DIM   16384
#define OCT_WARP_MAX_SHIFT (1 << 22)   /* |a|, |b|, |c| of kind 1 */
#define OCT_WARP_MAX_M     (1 << 20)   /* |m00|, |m01|, |m10|, |m11| of kind 2 */
typedef struct oct_warp_op {     /* one per sample of the batch, 40 bytes, in DEVICE memory */
    int kind;                    /* 0 none, 1 column shift, 2 affine */
    int border;                  /* 0 replicate, 1 wrap, 2 constant */
    int p[6];
    int fill;                    /* image value 0..255 of a tap outside the image (border 2) */
    int fill_label;              /* label value 0..255 outside the image (border 2) */
} oct_warp_op;
int oct_warp_batch(const unsigned char* x_u8_dev, const unsigned char* labels_dev, const oct_warp_op* ops_dev,
                   int B, int H, int W, int C,
                   unsigned char* x_out_dev, unsigned char* labels_out_dev, oct_stream_t stream);

/* ---- elastic deformation on device: (B,H,W,C) u8 images -> u8 images sampled through a smooth random displacement field;
 * (B,H,W) u8 labels moved alongside.  The U-Net paper's augmentation (Ronneberger et al. 2015, section 3.1); the reference has
 * no counterpart.  A stage of its own, in FRONT of oct_warp_batch: a sample may be deformed whatever warp, flip or noise it
 * then gets.  Integer arithmetic only, so the kernel, the numpy restatement (common/augmentation.py elastic_reference) and
 * the host generator give the same bytes.  Stand-alone: no handle, no allocation, one asynchronous launch on `stream`,
 * graph-capturable.  Per sample b, op = ops_dev[b]; `/` below is FLOOR division, `>>` an arithmetic shift, all intermediates
 * are 64-bit signed integers; the border rule is oct_warp_batch's.
 *   kind 0 none: copy.  kind 1 elastic, S = spacing:
 *   control grid: point (i, j), i = 0..(H-1)/S + 3, j = 0..(W-1)/S + 3, has the displacement (dx, dy) in 1/256 pixel
 *       r0..r3 = philox4x32_10(counter = (j, i, 0, 0x454C4153), key = (seed_lo, seed_hi))     (oct_augment_batch's generator)
 *       dx = (int)(((uint64)r0 (2 amp_x + 1)) >> 32) - amp_x,  dy likewise from r1 and amp_y: uniform integers in [-amp, amp].
 *   weights: pixel x has the cell cx = x / S and the offset k = x % S, and takes the uniform cubic B-spline of control columns
 *     cx..cx+3 with the numerators over 6 S^3
 *       b0 = (S-k)^3,  b1 = 3k^3 - 6Sk^2 + 4S^3,  b2 = -3k^3 + 3Sk^2 + 3S^2 k + S^3,  b3 = k^3     (all >= 0, sum 6 S^3);
 *     row y likewise with cy = y / S.
 *   displacement in 1/256 pixel, for dx and dy each:
 *       N = sum_a sum_b by_a bx_b d(cy + a, cx + b),   disp = (N + 18 S^6) / (36 S^6)              |disp| <= amp
 *   sampling: sx = 256 x + disp_x, sy = 256 y + disp_y (source position in 1/256 pixel)
 *     image: ix = sx >> 8, fx = sx & 255, iy, fy likewise; taps p00 = (ix, iy), p01 = (ix+1, iy), p10 = (ix, iy+1),
 *       p11 = (ix+1, iy+1), each through the border rule;
 *       out = ((256-fx)(256-fy) p00 + fx (256-fy) p01 + (256-fx) fy p10 + fx fy p11 + 32768) >> 16
 *     labels: the nearest pixel ((sx + 128) >> 8, (sy + 128) >> 8) through the border rule.
 *     amp_x = amp_y = 0 is the identity, byte for byte; amp_x = 0 is the axial-only deformation (pixels stay in their A-scan).
 *   Parameter ranges (OCT_ELASTIC_*): H, W <= 16384, S in 2..128, amp_x, amp_y in 0..8192 (32 pixels).  Then
 *     |N| <= 36 S^6 amp <= 36 2^42 2^13 < 2^61: no intermediate leaves int64, and every source index fits an int32.  The ranges
 *     are only visible on the device: REFUSE anything outside them on the host, before upload (common/augmentation.py
 *     check_elastic_ops).  A kind outside 0..1, or a border, spacing or amplitude outside its range, is TREATED AS kind 0 (no
 *     device-side flag).
 *   labels_dev == NULL or labels_out_dev == NULL: no labels written.  Nothing depends on b, B or the launch geometry.
 * Errors (negative, nothing launched): null x_u8_dev / ops_dev / x_out_dev, non-positive sizes, B > 65535, H or W >
 * 16384, H*W*C >= 2^31, labels_out_dev without labels_dev, an output range overlapping an input range or the other output
 * (the stage gathers: it cannot run in place). */
#define OCT_ELASTIC_MAX_DIM     16384
#define OCT_ELASTIC_MIN_SPACING 2
#define OCT_ELASTIC_MAX_SPACING 128
#define OCT_ELASTIC_MAX_AMP     8192     /* amp_x, amp_y: 32 pixels */
typedef struct oct_elastic_op {  /* one per sample of the batch, 40 bytes, in DEVICE memory */
    int kind;                    /* 0 none (the sample is copied through), 1 elastic */
    int border;                  /* 0 replicate, 1 wrap, 2 constant (oct_warp_batch's rule) */
    int spacing;                 /* S: control-point spacing in pixels, 2..128 */
    int amp_x, amp_y;            /* bound of the control displacements in 1/256 pixel, 0..8192 */
    unsigned seed_lo, seed_hi;   /* Philox key of this sample's field */
    int fill;                    /* image value 0..255 of a tap outside the image (border 2) */
    int fill_label;              /* label value 0..255 outside the image (border 2) */
    int reserved;                /* 0 */
} oct_elastic_op;
int oct_elastic_batch(const unsigned char* x_u8_dev, const unsigned char* labels_dev, const oct_elastic_op* ops_dev,
                      int B, int H, int W, int C,
                      unsigned char* x_out_dev, unsigned char* labels_out_dev, oct_stream_t stream);

/* ---- photometric augmentation on device: (B,H,W,C) u8 images -> u8 images of the same shape through a separable blur,
 * column shadows and an intensity table (gamma, brightness, contrast), per sample.  A training augmentation; the reference
 * has no counterpart.  A stage of its own directly BEHIND oct_elastic_batch and in front of oct_warp_batch.  Labels never
 * change, so the call takes none.  Integer arithmetic only, and the weights and the table are INPUT: the kernel, the numpy
 * restatement (common/augmentation.py photometric_reference) and the host generator give the same bytes whatever the host's
 * exp and pow do.  Stand-alone: no handle, no allocation, no atomics, one asynchronous launch on `stream`, graph-capturable.
 * Per sample b, op = ops_dev[b]; per pixel (y, x) and channel, in this order (`>>` a shift, `//` floor division):
 *   1. blur (kind & 1), R = radius: replicate border, clamp(i) = min(max(i, 0), n - 1) on the axis
 *        h(y, x) = sum_{k=-R..R} w[|k|] src(y, clamp(x + k))                         (<= 65280, kept exact)
 *        v0 = (sum_{j=-R..R} w[|j|] h(clamp(y + j), x) + 32768) >> 16;     without the flag v0 = src(y, x)
 *   2. shadows (kind & 2): g_s(x) = 256 - (strength_s max(0, hw_s - |x - cx_s|)) // hw_s for s < n_shadows;
 *        g(y, x) = min over the s with y >= y0_s of g_s(x), 256 when there is none;  v1 = (v0 g + 128) >> 8
 *   3. table (kind & 4): out = lut[v1];    without the flag out = v1
 *   kind 0: the sample is copied.
 *   Ranges (OCT_PHOTO_*): H, W <= 16384; kind 0..7; radius 0..8; w[0] + 2 sum_{k>=1} w[k] = 256 and w[k] = 0 for k > radius
 *     (then v0 <= 255); n_shadows 0..4; cx any int16 (it may lie outside the image); hw 1..4096; y0 0..16384; strength
 *     0..256 (then 0 <= g <= 256 and v1 <= v0); reserved 0.  The ranges are only visible on the device: REFUSE anything
 *     outside them on the host, before upload (common/augmentation.py check_photo_ops).  A kind outside 0..7, a radius above
 *     8, n_shadows above 4 or a live hw below 1 is TREATED AS kind 0 (no device-side flag); no other value can make the
 *     kernel read or write outside its buffers.
 *   Nothing depends on b, B or the launch geometry: repeated calls give identical bytes.
 * Errors (negative, nothing launched): null x_dev / ops_dev / out_dev, ops_dev not 4-byte aligned, non-positive sizes, B >
 * 65535, H, W or C > 16384, H*W*C >= 2^31, out_dev overlapping x_dev or ops_dev (the blur gathers: the stage cannot run in
 * place). */
#define OCT_PHOTO_BLUR        1
#define OCT_PHOTO_SHADOW      2
#define OCT_PHOTO_LUT         4
#define OCT_PHOTO_MAX_DIM     16384
#define OCT_PHOTO_MAX_RADIUS  8
#define OCT_PHOTO_MAX_SHADOWS 4
typedef struct oct_photo_op {    /* one per sample of the batch, 320 bytes, in DEVICE memory */
    int kind;                    /* flags: 1 blur, 2 shadows, 4 table; 0: the sample is copied through */
    int radius;                  /* R of the blur, 0..8 */
    unsigned short w[9];         /* blur weights: w[k] at offsets +-k */
    unsigned short n_shadows;    /* 0..4 */
    short cx[4];                 /* shadow centre column */
    short hw[4];                 /* shadow half-width in pixels, 1..4096 */
    short y0[4];                 /* first shadowed row, 0..16384 */
    unsigned short strength[4];  /* 0..256: the gain at the centre column is 256 - strength */
    unsigned reserved;           /* 0 */
    unsigned char lut[256];      /* the intensity table */
} oct_photo_op;
int oct_photo_batch(const unsigned char* x_dev, const oct_photo_op* ops_dev, int B, int H, int W, int C,
                    unsigned char* out_dev, oct_stream_t stream);

/* ---- edge weight map: per-pixel loss weights from the labels, on the device ----
 * weights[b, y, x] = lut[idx] of the capped squared distance to the nearest class border of image b -- the weight map of the
 * U-Net paper, w = 1 + w0 exp(-d^2 / 2 sigma^2), or ReLayNet's 1 + omega [x on a layer boundary], by the table the caller
 * uploads (common/utils.py edge_weight_lut).  Defined in integers (common/utils.py edge_weight_reference restates it):
 *   known:  label < n_cls.  The ignore label and every other byte >= n_cls are unknown.
 *   edge:   a known pixel with a 4-neighbour INSIDE the image that is known and has another label.  Both sides of a border
 *           are edge pixels; a border against unknown pixels (a pad frame, an unlabelled region) or the image rim is none.
 *   d2(x):  min of dx^2 + dy^2 over the edge pixels of the same image with dx^2 + dy^2 <= R^2;
 *           idx = d2, or R^2 + 1 ("far") where there is none; an edge pixel has idx 0.
 *   w(x):   lut[idx] for a known pixel, 0.0f for an unknown one.
 * lut_dev: R^2 + 2 floats.  labels_dev: (B,H,W) or (B,H,W,1) bytes; weights_dev: (B,H,W) f32.  Stand-alone: no handle, no
 * workspace, no allocation, one asynchronous launch on `stream`, graph-capturable, no atomics; two calls give the same bytes.
 * Errors (negative, nothing launched): null pointers, non-positive B, H or W, n_cls outside 1..255, radius outside
 * 1..OCT_EDGE_WEIGHT_MAX_RADIUS, B > 65535, H or W > OCT_EDGE_WEIGHT_MAX_DIM, lut_dev or weights_dev not 4-byte aligned,
 * weights_dev overlapping labels_dev. */
#define OCT_EDGE_WEIGHT_MAX_RADIUS 32
#define OCT_EDGE_WEIGHT_MAX_DIM    16384
int oct_edge_weight_map(const unsigned char* labels_dev, int B, int H, int W, int n_cls, int radius, const float* lut_dev,
                        float* weights_dev, oct_stream_t stream);

/* ---- contrast normalisation: CLAHE and percentile stretch of uint8 scans, on the device ----
 * x: (B,H,W,ch) bytes, ch in 1..4, every channel on its own; out: the same shape.  Defined in integers (common/utils.py
 * contrast_luts_reference / contrast_reference restate it and give the same bytes):
 *   tiles:   tile row r of tiles_y covers the image rows [r H / tiles_y, (r+1) H / tiles_y) (floor), tile columns alike;
 *            A = the tile's pixel count, h[0..255] its histogram of one channel.
 *   LUT of a tile, OCT_CONTRAST_CLAHE:
 *            L = A when clip_q8 = 0 (no limit), else max(1, (clip_q8 A) >> 16) in 64 bits -- clip_q8 / 256 is the limit in
 *            units of the uniform bin height A / 256;  E = sum_i max(h[i] - L, 0);  with r = E mod 256,
 *            h'[i] = min(h[i], L) + E / 256 + [(i+1) r / 256 > i r / 256]   (floors; one redistribution pass, the remainder
 *            spread evenly; a bin may exceed L again);  c[i] = sum_{j<=i} h'[j], c[255] = A;  lut[i] = (255 c[i] + A / 2) / A.
 *   LUT of a tile, OCT_CONTRAST_STRETCH:
 *            c = cumulative sum of h;  v_lo = min{i : c[i] > lo_bp A / 10000 (floor)},  v_hi = min{i : 10000 c[i] >= hi_bp A};
 *            the identity if v_hi <= v_lo, else lut[i] = 0 for i <= v_lo, 255 for i >= v_hi and between them
 *            ((i - v_lo) 255 + (v_hi - v_lo) / 2) / (v_hi - v_lo).
 *   apply:   Cy[r] = y0_r + y1_r - 1 is twice the centre of tile row r = [y0_r, y1_r).  For pixel row y:
 *            r = clamp(#{i : Cy[i] <= 2y} - 1, 0, max(tiles_y - 2, 0)), Dy = Cy[r+1] - Cy[r], ay = clamp(2y - Cy[r], 0, Dy);
 *            with tiles_y = 1: r = 0, ay = 0, Dy = 1 and the "next" row is row 0.  Columns alike: c, ax, Dx.  With v00, v01,
 *            v10, v11 the LUT values of the input byte in the tiles (r,c), (r,c+1), (r+1,c), (r+1,c+1):
 *            out = ((Dy-ay) ((Dx-ax) v00 + ax v01) + ay ((Dx-ax) v10 + ax v11) + Dy Dx / 2) / (Dy Dx)      (< 2^32 throughout).
 * Workspace: oct_contrast_workspace_bytes; 0 = this shape or descriptor is refused.  After the call its first
 * B * ch * tiles_y * tiles_x * 256 bytes are the LUTs in (B, ch, tiles_y, tiles_x, 256) order; what lies behind them is the
 * implementation's (the uint32 histograms).  out_dev == x_dev is allowed: the LUTs are finished before the apply pass and
 * one thread owns each byte.  No allocation, no host wait, asynchronous on `stream`, graph-capturable (one memset node and
 * three kernel nodes); the histograms are merged with integer atomics only, so repeated calls give the same bytes.
 * Errors (negative, nothing launched): null pointers; B outside 1..65535; H or W outside 1..OCT_CONTRAST_MAX_DIM; ch
 * outside 1..4; an unknown method; tiles outside 1..OCT_CONTRAST_MAX_TILES; H / tiles_y or W / tiles_x (floor) below
 * OCT_CONTRAST_MIN_TILE; clip_q8 neither 0 nor in 256..65535 (CLAHE); not 0 <= lo_bp < hi_bp <= 10000 (stretch); ws_bytes
 * too small; the workspace not 4-byte aligned; out_dev overlapping x_dev without being it; the workspace overlapping
 * x_dev or out_dev. */
#define OCT_CONTRAST_MAX_TILES 16
#define OCT_CONTRAST_MIN_TILE  8
#define OCT_CONTRAST_MAX_DIM   4096
enum { OCT_CONTRAST_CLAHE = 0, OCT_CONTRAST_STRETCH = 1 };
typedef struct oct_contrast_desc {
    int method, tiles_y, tiles_x;
    unsigned clip_q8;       /* CLAHE: round(clip * 256), 0 = no limit */
    int lo_bp, hi_bp;       /* stretch: the two percentiles in basis points */
} oct_contrast_desc;
size_t oct_contrast_workspace_bytes(int B, int H, int W, int ch, const oct_contrast_desc* d);
int oct_contrast_batch(const unsigned char* x_dev, int B, int H, int W, int ch, const oct_contrast_desc* d,
                       void* ws_dev, size_t ws_bytes, unsigned char* out_dev, oct_stream_t stream);

/* ---- pad and crop on device: scans whose size is no multiple of 2^pool_layers ----
 * oct_pad_batch places a (B,H,W,ch) batch -- uint8 (is_u8) or float32 -- at (top, left) of a (B,Hp,Wp,ch) batch of the same
 * type and fills the frame: out[b, y, x, :] = in[b, sy(y - top), sx(x - left), :] with, on an axis of length n,
 *   OCT_PAD_EDGE      s(i) = min(max(i, 0), n-1)                                    np.pad(mode="edge")
 *   OCT_PAD_REFLECT   s(i) = -i for i < 0, 2(n-1) - i for i >= n, else i            np.pad(mode="reflect"): no repeated edge
 *   OCT_PAD_CONSTANT  a pixel with i outside 0..n-1 on either axis is `value`       np.pad(mode="constant")
 * (uint8: `value` must be a whole number in 0..255; float32: `value` itself).  Hp == H, Wp == W is a copy.
 * oct_crop_batch is the inverse window: out[b, y, x] = in[b, y + top, x + left] over (B,Hp,Wp) pixels of `pixel_bytes`
 * bytes each -- 1 for arg-max maps, 4 for entropy / mutual information, 4 n_cls for probabilities; the kernel moves bytes.
 * (A pixel of more than 32 bytes, the probabilities of 9..16 classes, is cropped as 4-byte pixels of rows n_cls times as
 * long, with `left` scaled alike: oct_unet_infer and UNetEngine.crop do so.)
 * Stand-alone: no handle, no allocation, one asynchronous launch on `stream` each, graph-capturable.  common/utils.py
 * pad_reference / crop_reference restate them; padded_geometry there holds THE placement rule of the callers
 * (top = (Hp - H) / 2, left = (Wp - W) / 2, floor: the odd pixel goes to the bottom / right).
 * Errors (negative, nothing launched): null or overlapping buffers; non-positive B, H, W, ch, Hp, Wp; top or left < 0,
 * top + H > Hp, left + W > Wp; an unknown mode; reflect with a pad >= the image's dimension on that axis; a uint8 constant
 * that is no whole number in 0..255; float32 buffers that are not 4-byte aligned; pixel_bytes outside {1, 2, 4, 8, 12, ...,
 * 32}; element counts that overflow the kernels' indexing (B, Hp or the bytes of a row > 2^30, a buffer >= 2^62 bytes). */
#define OCT_PAD_EDGE     0
#define OCT_PAD_REFLECT  1
#define OCT_PAD_CONSTANT 2
int oct_pad_batch(const void* src_dev, int is_u8, int B, int H, int W, int ch, int Hp, int Wp, int top, int left, int mode,
                  float value, void* dst_dev, oct_stream_t stream);
int oct_crop_batch(const void* src_dev, int B, int Hp, int Wp, int pixel_bytes, int H, int W, int top, int left,
                   void* dst_dev, oct_stream_t stream);

/* ---- min-path boundary search on the device ----
 * The boundary delineation of min_path_processing/graph_search.py for (B, M, H, W) uint8 boundary maps as
 * oct_boundary_maps leaves them (M = classes - 1; no transpose), one workgroup per map.  The grid graph of the host
 * search is a DAG by columns -- interior vertices have edges only to the next column (right, max_grad up, max_grad
 * down), the zero-cost "down" edges exist only inside the two appended columns of ones -- so its shortest distances obey
 * a column recurrence, stated here and restated in numpy by min_path_processing/device_search.py::delineate_dp:
 *   p = k / 255 in fp64 (numpy's maps / 255; a 256-entry table divided on the host).  Graph column 0 and W + 1 are
 *   ones, graph column j + 1 is image column j.  D[0][r] = 0.  For j = 0..W-1 and every row r,
 *     D[j+1][r] = min over r' in {r, r+1..r+max_grad, r-1..r-max_grad} within [0, H) of
 *                 D[j][r'] + (2.0 - (P[j][r'] + P[j+1][r])),            all fp64, no contraction.
 *   Every edge weight is >= 0 and fp64 addition is monotone: D equals, bit for bit, Dijkstra's final distances.
 *   Equal predecessors: the FIRST that attains the minimum in the order right (r), below nearest first (r+1, r+2, ..),
 *   above nearest first (r-1, ..) is chosen; the vertex carries a tie bit if more than one attains it and j >= 1 (the
 *   predecessors in the appended column 0 are all equal and change no delineation).
 *   End: cost = min over r' of D[W][r'] + (2.0 - (P[W][r'] + 1.0)), the smallest such r'; tied if more than one attains it.
 *   Back-trace from (W, r') to graph column 1: rows_out[image column] = row; the map's tie flag is the OR of the end
 *   tie and the tie bits of the vertices on the chosen path (a tie bit off the path cannot change it; another optimal
 *   delineation shows as a tie bit where the two paths merge).
 * tied_out = 0: the minimum-cost delineation is unique and rows_out is what the host search returns.  tied_out = 1: the
 * host search resolves the tie by the push order of its heap, which no column rule reproduces -- send that map to the
 * host, or accept the rule above.  cost_out equals the host search's distance of the end vertex for every map.
 * oct_minpath_workspace_bytes: bytes of workspace for up to B images, 0 for an unsupported shape (H or W beyond the
 * uint16 rows, max_grad outside 1..16, or H beyond what one workgroup's LDS holds: two fp64 column pairs and a map tile,
 * about 1600 rows).  The predecessor bytes (W x H per map) stay in LDS when they fit (256 x 512 does) and use the
 * workspace otherwise.  oct_minpath_device: stand-alone, no handle, no allocation, no host synchronisation, one
 * asynchronous launch on `stream`, graph-capturable (call once outside a capture first when W * H exceeds 32 KiB: the
 * first launch per device raises the kernel's dynamic LDS limit).  Errors (negative, nothing launched): null pointers,
 * max_grad outside 1..16, an unsupported shape, a workspace smaller than oct_minpath_workspace_bytes. */
size_t oct_minpath_workspace_bytes(int B, int M, int H, int W, int max_grad);
int oct_minpath_device(const unsigned char* maps_dev, int B, int M, int H, int W, int max_grad,
                       void* workspace_dev, size_t workspace_bytes,
                       unsigned short* rows_out_dev /* (B, M, W) */, double* cost_out_dev /* (B, M) */,
                       unsigned char* tied_out_dev /* (B, M) */, oct_stream_t stream);

/* ---- evaluation Dice on the device (csrc/kernels_dice.hpp; host restatements: evaluation/dice_device.py) ----
 * Both calls are stand-alone (no handle), allocate nothing, are asynchronous on `stream`, never wait for it and record
 * into a stream capture.  Argument errors return a negative code with oct_last_error() and launch nothing.
 *
 * oct_confusion_counts: counts[b][g * n_cls + p] = number of pixels of image b with gt == g and pred == p, for (B,H,W)
 * uint8 class maps; the last word of a row counts the pixels where either label is >= n_cls, which appear nowhere else
 * in the row.  The call overwrites counts_dev (zeroing is part of it).  1 <= B <= 65535, H*W < 2^32, 2 <= n_cls <= 32.
 * Every Dice metric of the evaluation is a function of one row (dice_from_counts).
 *
 * oct_confusion_counts_masked: the same for partially labelled ground truth, rows of n_cls*n_cls + 2 words.  A pixel with
 * gt == ignore_label (a value in n_cls..255) is counted in word n_cls*n_cls + 1 and nowhere else, whatever its prediction;
 * words 0..n_cls*n_cls-1 are the confusion matrix of the other pixels and word n_cls*n_cls counts those of them where
 * either label is >= n_cls.  Limits as above; ignore_label outside n_cls..255 is an argument error.
 *
 * oct_area_labels: the class map, in the (H,W) frame, that graph-search delineations enclose -- exactly
 * common/utils.py::labels_from_delineations.  Per column, with M = n_cls - 1 and s_i = segs[b][i][col]: going up in i,
 * s_i == 0 becomes the first non-zero s_j with j > i, or H; row r then gets M if r >= s_{M-1}, else the largest k in
 * 1..M-1 with s_{k-1} <= r < s_k, else 0.  Boundaries may cross; values >= H reach no row.  H <= 65535, else as above. */
int oct_confusion_counts(const unsigned char* pred_dev, const unsigned char* gt_dev, int B, int H, int W, int n_cls,
                         unsigned int* counts_dev /* (B, n_cls*n_cls + 1) */, oct_stream_t stream);
int oct_confusion_counts_masked(const unsigned char* pred_dev, const unsigned char* gt_dev, int B, int H, int W, int n_cls,
                                int ignore_label, unsigned int* counts_dev /* (B, n_cls*n_cls + 2) */, oct_stream_t stream);
int oct_area_labels(const unsigned short* segs_dev /* (B, n_cls-1, W) */, int B, int H, int W, int n_cls,
                    unsigned char* labels_dev /* (B, H, W) */, oct_stream_t stream);

/* ---- calibration on the device (csrc/kernels_calibration.hpp; numpy restatement: evaluation/calibration.py; the reference has
 * no counterpart: nothing there asks whether its softmax output is a probability) ----
 * Three calls on class probabilities probs_dev (B, npix, n_cls) float32 -- the (B,H,W,n_cls) tensor the head, oct_mc_update or
 * oct_tta_update leave on the device, npix = H*W -- two of them against ground-truth labels_dev (B, npix) uint8.  A pixel is
 * COUNTED iff its label y < n_cls and y != ignore_label (-1: none, else 0..255).  EPS = 1e-7f (FOCAL_EPS of the losses).  Every
 * per-pixel step is one IEEE fp32 operation, sums over classes run in class order, nothing is contracted, logf / expf are the
 * OCML library functions; every sum over pixels is fp64.
 *
 * oct_calibration_counts, per image over its counted pixels, with M = n_bins in 1..64:
 *   m    = the lowest index of the maximum of p          conf = min(max(p_m, 0), 1)
 *   k    = (uint32) floor(conf * 2^28)                   (the product is exact: a power of two)
 *   bin  = min(M - 1, (uint64(k) * M) >> 28)             (integers: a confidence on a bin edge has one answer; 1.0 -> M - 1)
 *   counts[b][bin] += (1, m == y, k)                     counts_dev: uint64 (B, M, 3) = pixels, correct pixels, sum of k
 *   nll   = -logf(min(max(p_y, EPS), 1 - EPS))           (1 - EPS in fp32; the cross-entropy of the focal and BCE terms)
 *   brier = sum_c (p_c - [c == y])^2                     (fp32: subtract, square, add in class order)
 *   sums_dev: float64 (B, 4) = sum nll, sum brier, counted pixels, pixels with y >= n_cls that are not ignore_label.
 *   The integer words do not depend on any order and are compared bit for bit with the restatement; the fp64 sums are
 *   reduced thread -> wave -> block -> image in a fixed order, so repeated calls give identical bytes.  The confidence of a
 *   distribution over <= 32 classes is >= 2^-5, hence a multiple of 2^-28: for such input k loses nothing.
 *
 * oct_temperature_apply, per pixel of (npix_total, n_cls), beta = 1 / T finite and > 0:
 *   l_c = logf(max(p_c, EPS))   L = max_c l_c   e_c = expf(beta * (l_c - L))   S = e_0 + e_1 + ...   q_c = e_c / S
 *   i.e. softmax(logits / T) formed from the probabilities alone.  probs_out_dev may be probs_in_dev (a pixel is owned by one
 *   thread); any other overlap is an error.
 *
 * oct_temperature_nll, per image over its counted pixels and for each of the K = n_betas <= 8 values betas[k] (a HOST array,
 * read during the call), with l, L, e, S, q as above:
 *   nll = logf(S) - beta * (l_y - L)
 *   mu  = q_0 * l_0 + q_1 * l_1 + ...                    g = mu - l_y
 *   h   = q_0 * ((l_0 - mu) * (l_0 - mu)) + ...          (the centred form: E[l^2] - E[l]^2 cancels)
 *   out_dev: float64, (B, K, 3) sums of nll, g, h, then (B) counted pixels.  g and h are the first and second derivative in
 *   beta of the summed NLL, which is convex in beta.  The row of a beta does not depend on K or on its position.
 *
 * All are stand-alone like oct_mc_update: no handle, no allocation, asynchronous on `stream` (counts and nll: a launch over the
 * pixels that leaves one partial row per block in the caller-owned workspace, and a small one that adds the rows per image;
 * no global atomics), never wait, record into a stream capture.  Pointers need their natural alignment (outputs and
 * workspace: 8 bytes); with 16-byte aligned probabilities, n_cls <= 8 and npix*n_cls % 4 == 0 the kernels move float4s.
 * Errors (negative, oct_last_error(), nothing launched): null pointers, B outside 1..65535, npix < 1, B*npix >= 2^31, n_cls
 * outside 2..32, n_bins outside 1..64, n_betas outside 1..8, a beta that is not finite and positive, ignore_label outside
 * -1..255, a workspace smaller than the _workspace_bytes of the call, misaligned buffers, overlapping ranges.  The
 * _workspace_bytes functions return 0 for a shape the calls refuse. */
size_t oct_calibration_workspace_bytes(int B, size_t npix, int n_cls, int n_bins);
int oct_calibration_counts(const float* probs_dev /* (B, npix, n_cls) f32 */, const unsigned char* labels_dev /* (B, npix) */,
                           int B, size_t npix, int n_cls, int ignore_label, int n_bins,
                           unsigned long long* counts_dev /* (B, n_bins, 3) */, double* sums_dev /* (B, 4) */,
                           void* ws_dev, size_t ws_bytes, oct_stream_t stream);
int oct_temperature_apply(const float* probs_in_dev, float* probs_out_dev /* (npix_total, n_cls) f32 */, size_t npix_total,
                          int n_cls, float beta, oct_stream_t stream);
size_t oct_temperature_workspace_bytes(int B, size_t npix, int n_cls, int n_betas);
int oct_temperature_nll(const float* probs_dev, const unsigned char* labels_dev, int B, size_t npix, int n_cls, int ignore_label,
                        const float* betas /* host, n_betas values */, int n_betas,
                        double* out_dev /* (B, n_betas, 3) then (B) */, void* ws_dev, size_t ws_bytes, oct_stream_t stream);

/* ---- ordered layer decode on the device (csrc/kernels_ordered.hpp; numpy restatement: common/utils.py::
 * ordered_decode_reference; the reference has no counterpart: between its arg-max and its result files only the per-boundary
 * min-path search repairs a column whose classes are out of depth order) ----
 * probs_dev (B, H, W, n_cls) float32, class index == depth order.  For one column (b, x), rows r = 0..H-1, C = n_cls:
 *   q        = p > 0 ? min(p, 1) : 0                          (NaN -> 0)
 *   k[r][c]  = min((uint32) floor(q * 2^20), 2^20 - 1)        (the product is exact; H <= 4096 keeps every sum below 2^32)
 *   F[r][c]  = k[r][c] + M[r-1][c],   M[-1][c] = 0            (uint32)
 *   M[r][0]  = F[r][0],  s[r][0] = 1
 *   M[r][c]  = F[r][c] if F[r][c] > M[r][c-1] (s[r][c] = 1) else M[r][c-1] (s[r][c] = 0)        c = 1..C-1
 *   back-trace: c = C-1;  for r = H-1 down to 0:  while (c > 0 && !s[r][c]) c--;  label[r] = c
 *   score    = M[H-1][C-1]
 *   rows[i]  = number of rows with label <= i,  i = 0..C-2    (the first row of a class > i; H if there is none)
 * The labelling maximises sum_r k[r][label[r]] over all labellings that never decrease with r -- the expected number of
 * correctly labelled pixels of the column -- and classes may be skipped (layers of zero thickness).  Among the optima it is the
 * one that is smallest when compared from the bottom row upward (`>` is strict: a tie goes to the lower class).
 * labels_out_dev (B,H,W) uint8, rows_out_dev (B, n_cls-1, W) uint16, score_out_dev (B, W) uint32; each may be NULL, not all.
 * THE LABEL MAP IS AUTHORITATIVE.  rows[i] == 0 says that the column starts below boundary i; consumers of delineations
 * (oct_area_labels, the renderer, calc_errors) read 0 as "nothing here", so oct_area_labels(rows) reproduces the label map in
 * the columns where every row is in 1..H-1 (and where a row is H: the classes behind it are absent from the bottom); in a
 * column with a row of 0 it takes the boundary for missing, fills it from the next one below, and so names the column's top
 * stretch with a lower class than the label map does.
 * Stand-alone like oct_calibration_counts: no handle, no allocation, no atomics, ONE launch, asynchronous on `stream`, never
 * waits, records into a stream capture; repeated calls give identical bytes.  A thread owns one column (under option "ordered_float4", oct_set_option, four adjacent
 * ones where probs_dev is 16-byte aligned, n_cls <= 8 and W*n_cls % 4 == 0: float4 loads) and walks it twice: down, leaving the
 * n_cls decision bits of every (row, column) as a uint16 in the caller-owned workspace, and up, reading them back.
 * Errors (negative, oct_last_error(), nothing launched): null probs or workspace, all three outputs null, B, H or W < 1, n_cls
 * outside 2..16, H > 4096, B*H*W >= 2^31, a workspace smaller than oct_ordered_workspace_bytes (which returns 0 for a shape the
 * call refuses) or not 8-byte aligned, misaligned buffers, an output overlapping the input, the workspace or another output. */
size_t oct_ordered_workspace_bytes(int B, int H, int W, int n_cls);
int oct_ordered_decode(const float* probs_dev /* (B, H, W, n_cls) f32 */, int B, int H, int W, int n_cls, void* ws_dev, size_t ws_bytes,
                       unsigned char* labels_out_dev /* (B, H, W) or NULL */, unsigned short* rows_out_dev /* (B, n_cls-1, W) or NULL */,
                       unsigned int* score_out_dev /* (B, W) or NULL */, oct_stream_t stream);

/* ---- connected components of a class map on the device (csrc/kernels_components.hpp; numpy restatements: common/utils.py::
 * components_reference and component_filter_reference; the reference has no counterpart) ----
 * labels_dev (B, H, W) uint8.  Integers throughout; the restatements and the kernels agree bit for bit.
 *   neighbours   two pixels of ONE image with |dy| + |dx| == 1 (connectivity 4) or max(|dy|, |dx|) == 1 (connectivity 8).
 *   component    a maximal set of pixels of equal byte value joined by chains of neighbours.  Any byte value 0..255 forms
 *                components; n_cls bounds only the statistics.  Components never join across images.
 *   root[b,y,x]  the smallest y*W + x over the pixel's component: canonical, whatever the order of the merges.
 *   size[b,y,x]  the pixel count of the component at its root pixel, 0 at every other pixel.
 *   stats[b,c]   (number of components of class c in image b, pixels of the largest one); (0, 0) when the class is absent; c < n_cls.
 * root_out_dev (B,H,W) uint32; size_out_dev (B,H,W) uint32 or NULL; stats_out_dev (B, n_cls, 2) uint32 or NULL.
 * Stand-alone like oct_ordered_decode: no handle, no allocation, asynchronous on `stream`, never waits, records into a stream
 * capture; repeated calls give identical bytes.  The launches depend on the shape and on which outputs are wanted, never on
 * the data: a memset of the statistics, a union-find per 64x64 tile in LDS, a union across the tile borders (skipped for an
 * image of one tile; every access to the parent words there is a relaxed agent-scope atomic), a pass that flattens every pixel
 * to its root and moves the counts there, and one that forms the statistics.  Integer atomicMin / atomicAdd / atomicMax whose
 * final value does not depend on the order; no thread waits for another, every find / union loop follows strictly decreasing
 * indices.  The workspace (8-byte aligned) holds the size words when size_out_dev is NULL, and the filter's scratch.
 * Errors (negative, oct_last_error(), nothing launched): null labels, root or workspace, B outside 1..65535, H or W < 1,
 * B*H*W >= 2^31, n_cls outside 1..32, a connectivity other than 4 or 8, a workspace smaller than
 * oct_components_workspace_bytes (which returns 0 for a shape the call refuses) or misaligned, misaligned outputs, an output
 * overlapping the input, the workspace or another output.
 *
 * oct_component_filter reads labels_dev and the root and size words of oct_components and writes the cleaned map, out of place.
 *   removed      a pixel of class c < n_cls with root r is REMOVED if size[r] < rule->min_pixels[c], or if bit c of
 *                rule->keep_largest is set and r is not the best root of (b, c): the component of class c with the most pixels,
 *                among equals the one with the smallest root.  Pixels with a label >= n_cls are never removed.
 *   kept         a kept pixel keeps its byte.
 *   fill mode 0  a removed pixel gets rule->fill_label.
 *   fill mode 1  a removed pixel gets the label of the nearest pixel ABOVE it in its column that is kept and has a label
 *                < n_cls; if there is none, that of the nearest such pixel below it; if there is none, rule->fill_label.  The
 *                rule that suits B-scans: a speck takes the class of the layer over it.
 *   removed[b,c] the removed pixels whose original class is c; removed_out_dev (B, n_cls) uint32 or NULL.
 * ONE pass and NOT idempotent: filled regions may join their neighbours, so the components of the cleaned map are not those of
 * the input less the removed ones; run oct_components again on the cleaned map before filtering it again.  The workspace bytes
 * are those of oct_components_workspace_bytes; the launches depend on the rule alone (the best roots only if keep_largest != 0,
 * the column walk -- a thread per column -- only under fill mode 1).  Otherwise as oct_components.
 * Errors: as oct_components, and null size, rule or output, a fill mode outside 0..1, a fill label outside 0..255,
 * keep_largest bits at or above n_cls. */
typedef struct oct_component_rule {   /* HOST struct, copied into the kernel arguments by the call */
    unsigned int min_pixels[32];      /* class c: components with fewer pixels are removed (0 or 1: none) */
    unsigned int keep_largest;        /* bit c: of class c only the largest component of each image stays */
    int fill_mode;                    /* 0 constant, 1 column */
    int fill_label;                   /* 0..255 */
} oct_component_rule;
size_t oct_components_workspace_bytes(int B, int H, int W);      /* 0 = a shape the call refuses */
int oct_components(const unsigned char* labels_dev /* (B, H, W) */, int B, int H, int W, int n_cls, int connectivity /* 4 | 8 */,
                   void* ws_dev, size_t ws_bytes, unsigned int* root_out_dev /* (B, H, W) */,
                   unsigned int* size_out_dev /* (B, H, W) or NULL */, unsigned int* stats_out_dev /* (B, n_cls, 2) or NULL */,
                   oct_stream_t stream);
int oct_component_filter(const unsigned char* labels_dev, const unsigned int* root_dev, const unsigned int* size_dev,
                         int B, int H, int W, int n_cls, const oct_component_rule* rule, void* ws_dev, size_t ws_bytes,
                         unsigned char* labels_out_dev /* (B, H, W) */, unsigned int* removed_out_dev /* (B, n_cls) or NULL */,
                         oct_stream_t stream);

/* ---- PNG pictures on the device (csrc/kernels_render.hpp; numpy restatement: common/plotting.py::render_reference) ----
 * oct_render_rgba renders B images of H x W into out_dev (B, H, W, 4) uint8 RGBA with A = 255: a base layer, then
 * K >= 0 polylines over it.  Integers only; the restatement and the kernel agree bit for bit.
 *
 * Base layer.  OCT_RENDER_BASE_IMAGE: base_dev is (B, H, W, ic) uint8; ic == 3 gives R, G, B, any other ic gives
 * R = G = B = channel 0.  OCT_RENDER_BASE_LABELS: base_dev is (B, H, W) uint8 (ic is ignored) and a pixel gets
 * style->palette[label], a label >= style->n_cls gives (0, 0, 0).
 *
 * Lines.  rows_dev is (B, K, W) uint16, K = style->n_lines (rows_dev may be NULL when K == 0); line k has the colour
 * style->line_rgb[3k..3k+2] and the style style->line_style[k], 0 solid or 1 dotted.  Lines are drawn in index order.
 * One inclusive column range [col_lo, col_hi] and one half_width R in eighths of a pixel (1..64; 22 = a 5.5 px line)
 * hold for the whole call.  In eighths of a pixel, the centre of pixel (r, c) at (x, y) = (8c, 8r):
 *   vertex    column c of a line has a vertex at (8c, 8 rows[c]) iff col_lo <= c <= col_hi and 0 < rows[c] < H
 *             (0 is the searches' "nothing here"; a row >= H counts as missing too).
 *   segment   columns c and c+1 form a segment iff both have a vertex; an isolated vertex draws nothing.
 *   samples   a pixel has 16 samples s = (8c + ox, 8r + oy), ox, oy in {-3, -1, 1, 3}.
 *   on        for the segment P0 -> P1, d = P1 - P0 = (8, 8 (rows[c+1] - rows[c])), w = s - P0, t = w.d, den = d.d:
 *             t <= 0: |w|^2 <= R^2;  t >= den: |s - P1|^2 <= R^2;  otherwise |w|^2 den - t^2 <= R^2 den
 *             (round caps and joins).  All of it fits int64 for H <= 4096.
 *   dotted    a sample counts only when floor_mod(sx - 8 col_lo, 120) < 48: 6 px on in a period of 15, phased by column.
 *   coverage  the number of the pixel's samples, 0..16, that are on ANY segment of the line (joins do not count twice).
 *   blend     per channel out = (cov * colour + (16 - cov) * out + 8) >> 4, line after line.
 * So an interior flat solid line of R = 22 at row y covers rows y-2..y+2 fully and rows y-3, y+3 with coverage 4, and a gap
 * narrower than the line closes under the round caps.
 *
 * The palette, the line colours and the line styles travel BY VALUE: `style` is a host struct that the call copies into the
 * kernel's arguments before it returns (nothing of it is read later, no device buffer is involved).  Stand-alone like
 * oct_area_labels: no handle, no allocation, one asynchronous launch on `stream`, never waits, records into a stream
 * capture.  Errors (negative, oct_last_error(), nothing launched): null pointers, non-positive sizes, B > 65535, an unknown
 * base mode, n_cls outside 1..32 in label mode, K outside 0..16, H > 4096, half_width outside 1..64, col_lo > col_hi or a
 * range outside 0..W-1, an output range overlapping an input. */
#define OCT_RENDER_BASE_IMAGE 0
#define OCT_RENDER_BASE_LABELS 1
#define OCT_RENDER_MAX_CLASSES 32
#define OCT_RENDER_MAX_LINES 16
typedef struct oct_render_style {
    int n_cls;                                              /* label mode: entries of palette in use */
    int n_lines;                                            /* K */
    int col_lo, col_hi;                                     /* inclusive column range of every line */
    int half_width;                                         /* R, eighths of a pixel */
    unsigned char palette[3 * OCT_RENDER_MAX_CLASSES];      /* RGB per class */
    unsigned char line_rgb[3 * OCT_RENDER_MAX_LINES];       /* RGB per line */
    unsigned char line_style[OCT_RENDER_MAX_LINES];         /* 0 solid, 1 dotted */
} oct_render_style;
int oct_render_rgba(int base_mode, const unsigned char* base_dev, int ic, const unsigned short* rows_dev /* (B, K, W) */,
                    const oct_render_style* style /* host */, int B, int H, int W,
                    unsigned char* out_dev /* (B, H, W, 4) */, oct_stream_t stream);

/* ---- options ----
 * oct_set_option edits the PROCESS-WIDE DEFAULTS; a handle copies them when it is created (oct_unet_create) and every
 * launch of that handle reads its own copy: changing an option never affects a live handle, and two handles created
 * under different settings coexist in one process.  oct_unet_workspace_bytes uses the defaults current at the call, so
 * size and create a handle under the same settings.  oct_unet_get_option reads a handle's copy.
 * Three select ARITHMETIC (documented alternatives, each tested against the oracle):
 *   "mfma_mode" (default 1): 1 = convolutions on the bf16 matrix pipe -- in fp32 mode (cfg.dtype 0) every fp32 operand is
 *   split exactly into three bf16 terms and a product is six bf16 MFMAs accumulated in fp32 (fp32-equivalent results,
 *   DESIGN.md section 4); in bf16 mode (cfg.dtype 1) activations and weights are rounded once and multiplied directly.
 *   0 = the fp32-pipe kernels (v_mfma_f32_*_f32), fp32 math on whatever the storage type is.
 *   "focal_clip_modulation" (default 0): see oct_unet_set_focal_dice.
 *   "bce_inner_eps" (default 1): see oct_unet_set_bce_dice.
 * The rest are tuning knobs (results do not depend on them beyond fp32 rounding, only which kernel variant runs):
 *   "bx_min_blocks" (256): a wide bf16-pipe launch takes the taller pixel tile only if that still yields this many blocks.
 *   "bx_two_blocks" (1): wide bf16-pipe launches (3x3 and 2x2-over-upsample) run as 4-wave blocks with ONE input image in LDS,
 *   two blocks per CU -- each block's prologue, barriers and epilogue hide behind the other's MFMAs; 0 = the 8-wave blocks
 *   with a double-buffered image, one per CU (then "bx_min_blocks" / "bx_waves" pick their tile height and wave count).
 *   "fuse_dw_thin" (1): 3x3 layers with 8 output channels (the full-resolution convs): the backward-data launches also
 *   reduce the layer's backward-weights (conv_bt_k FDW); 0 = a separate backward-weights kernel.
 *   "bx_waves" (8 | 4): waves per block of conv_bx_k where the tile has >= 8 rows (two / one per SIMD).
 *   "dwbx_blocks" (256): grid target of the wide bf16-pipe backward-weights kernel.
 *   "bt_blocks_per_cu" (0 = as many as the LDS images allow): persistent blocks of the thin bf16-pipe kernel.
 *   "bt_m2" (1): thin bf16-pipe launches with exactly 8 output channels use the two-pixel form (16 MFMA rows = 2 adjacent
 *   pixels x 8 channels); read when the handle is created (the weights are prepared in that form).  0 = one pixel per column.
 *   "fuse_first_apply" (1): the first conv's BN-backward transform is applied inside its backward-weights kernel (the
 *   only consumer of that dz) instead of by a bn_bwd_apply pass; bit-identical gradients; oct_unet_debug_activation(0, 1)
 *   then returns the masked gradient g' of block 0, not dz.  0 = separate pass.
 *   "fuse_bn_apply" (1): every other block's BN-backward transform dz = ga g' + gb z + gd is applied by the consumers of
 *   dz -- its backward-weights kernel and its backward-data launches -- while they stage g' and z, wherever all of them
 *   can (the bf16-pipe conv kernels; every MFMA backward-weights kernel); the bn_bwd_apply pass (3 tensor passes per
 *   block) disappears.  Same two fmas per element as the stand-alone pass: bit-identical gradients.  The block's g buffer
 *   then keeps g' (oct_unet_debug_layer_fused tells which blocks).  0 = separate pass everywhere.
 *   "fuse_bn_apply16" (1): ... including the thin backward-data launches with 16 K and 16 output channels (their transform
 *   coefficients live in LDS: the registers are taken by two raw tiles, the mask input and the weights); 0 = those blocks
 *   keep the separate pass (same step time at B = 32, 256x512; 0.2 GB more HBM traffic per step).
 *   "fuse_bn_finalize" (0): 1 = the BN records of the thin layers (<= 32 channels) are written by the LAST block of the
 *   launch that produces the partial rows (arrival counter; write-through rows; csrc/kernels_fin.hpp) instead of by a
 *   bn_*_finalize launch.  Same results to fp32 rounding; measured 0.5-1 % slower per step than the launches it removes,
 *   hence off by default.  (The channel-streaming head kernels never finalize in the launch: under "head_wide", and above
 *   32 channels, the last block's statistics are finalized by the bn_bwd_finalize launch whatever this option says.)
 *   "pool_in_epilogue" (1; fp32 storage only; may be set on a live handle between steps): the bf16-pipe forward conv in
 *   front of a max-pool also writes the pooled tensor, from its accumulators, as the RAW window extrema of z -- the maximum
 *   where the layer's gamma >= 0 (+-0 included), the minimum where gamma < 0 -- and the pool's consumers (the next conv and
 *   its backward-weights kernel) apply the producer's BN + ReLU on load.  relu(fma(a, z, b)) is monotone in z with the
 *   direction of sign(gamma), so this is bit for bit what pool_fwd_k computes from relu(a z + b), without re-reading z.
 *   conv_bt_k does it (8 and 16 K channels), and conv_bx_k where a wave holds two tile rows; the other producers (the wide form with
 *   one tile row per wave, the fp32-pipe kernels, the image layer) and bf16 storage keep the pool_fwd_k pass.  0 = that
 *   pass everywhere.
 *   "bx_down2_ring" (1; may be set on a live handle between steps): the stride-2 forms of conv_bx_k (backward-data of the
 *   up-convolutions) run as many blocks as are resident at once; a block walks a strided list of (image, tile) items and
 *   requests, converts and copies the first K chunk of its next item while the last tap row of the current one is
 *   multiplied ("persistent_max_blocks" caps that grid).  0 = one block per item.  Every item keeps its own accumulators,
 *   epilogue and statistic row: results are bit for bit the same either way.
 *   "head_wide" (0; may be set on a live handle between steps): the head (BN + ReLU on load, 1x1 conv, softmax, loss
 *   sums; backward: loss gradient, softmax Jacobian, 1x1 backward, mask, statistics) has two forms.  The register kernels
 *   head_fwd_k / head_bwd_k<C, CIN> keep a pixel's CIN channels and CIN*C + C + 2*CIN partial sums in registers and exist
 *   for start_neurons <= 32.  The channel-streaming kernels head_fwd_wide_k / head_bwd_wide_k<C> (csrc/kernels_head_wide.hpp)
 *   take CIN at run time, stream z in 16-byte steps and form the sums over pixels on the fp32 matrix pipe; start_neurons
 *   36..64 always run them.  1 = every start_neurons runs them (same buffers, same arithmetic per pixel, another -- fixed --
 *   summation order), so that they can be tested and timed against the register kernels on equal inputs.
 *   "dwbt_f32_all" (0): 1 = fp32 mode takes conv_dwbt_k for every thin backward-weights shape (default: where it wins).
 *   "dw_side_stream" (1): backward-weights kernels and the per-step weight preparation run on a low-priority stream
 *   owned by the handle, beside the backward-data chain.  0 = everything on the caller's stream.
 *   "fork_on_launch" (1): the event such a backward-weights kernel waits for is the completion signal of the preceding
 *   launch itself (hipExtLaunchKernelGGL stopEvent) rather than a marker recorded behind it.  "dw_fork_group" (1): blocks
 *   whose backward-weights launches share one fork (2-4: fewer waits on the caller's stream, measured slower overall).
 *   "event_sysfence" (0; read at oct_unet_create): 1 = the handle's internal fork/join events carry a system-scope fence.
 *   "ordered_float4" (0; read by every oct_ordered_decode call): 1 = a thread takes four adjacent columns and loads their
 *   4 n_cls floats of a row as n_cls float4s, where probs_dev is 16-byte aligned, n_cls <= 8 and W*n_cls % 4 == 0.  Measured
 *   slower than one column per thread at every shape tried; kept so that the two forms can be tested and
 *   timed on equal inputs.  The results do not depend on it.
 *   Experiment switches, not for production use: "dwbx_enable" (1; 0 routes the wide backward-weights layers to the
 *   fp32-pipe kernel) and "timing_skip" (0; bit 0 / 1 SKIP the forward / backward BN finalize launches after the second
 *   step -- the results are then WRONG; used once to measure what those launches cost).
 *   "igemm_persistent_min_tiles" (default 2048): number of pixel tiles from which thin single-chunk convs use the
 *   persistent software-pipelined kernel instead of the one-tile-per-block kernel.
 *   "thin8_min_tiles" (default 2048): number of pixel tiles from which 8-output-channel convs run on the VALU
 *   thin-layer kernel instead of the (half-padded) 16x16 MFMA kernel.
 *   "pair8_min_tiles" (default 2048): number of pixel tiles from which 3x3 convs with 8 output channels run on the
 *   pixel-pair MFMA kernel (takes precedence over the VALU kernel).
 *   "dw32_blocks" (512) / "dw16_blocks" (768): target block count of a backward-weights launch (wide / thin kernels; one
 *   partial slab per block -- read when the handle is created, later launches never exceed the slabs allocated then).
 *   "igemm_persistent_blocks" (1280): grid of the persistent igemm kernel.  "igemm_min_blocks" (512): a layer takes the
 *   taller pixel tile only if that still yields this many blocks.
 *   "dwpair8_enable" (default 1): backward-weights of 3x3 layers with 8 output channels on the pixel-pair kernel
 *   (0 = the padded 16-column kernel).
 *   "pair8_geometry" (NWY*100 + NWX*10 + RPW in {221, 111}, default 221): waves per block (rows x columns)
 *   and 4-row groups per wave of that kernel; its tile is (4*RPW*NWY) x (32*NWX) pixels.
 *   "persistent_max_blocks" (default 0 = no cap; 0 .. 1 << 20, anything else is an error): for tests: caps the grid of
 *   every persistent launch so that small images make blocks walk several tiles.  The statistic rows and backward-weights
 *   slabs of a launch follow the capped grid.  May be set on a live handle. */
int oct_set_option(const char* name, int value);
int oct_get_option(const char* name, int* value);
int oct_unet_get_option(const oct_unet* h, const char* name, int* value);
/* edit a live handle's copy (between steps).  Everything but "bt_m2" (it shapes the prepared weights); launches never use
 * more partial-slab rows than were allocated at creation, whatever the block-count knobs say later. */
int oct_unet_set_option(oct_unet* h, const char* name, int value);

/* ---- introspection for tests: device pointer of a layer's saved pre-BN output / gradient ---- */
/* which: 0 = z, 1 = g (f32 or bf16 per cfg.dtype; max_batch x out_h x out_w x cout);
 *        2 = the layer's BN record, f32 [9][cout]: a, b (y = relu(a*z + b)), batch/moving mean, rstd, c1, c2 and the
 *            BN-backward transform dz = ga g' + gb z + gd as rows ga, gb, gd */
const void* oct_unet_debug_activation(oct_unet* h, int layer, int which);
/* 1 if, in the last oct_unet_backward, the layer's BN-backward transform was applied on load by its consumers (its g
 * buffer still holds the masked gradient g'), 0 if the stand-alone pass turned g into dz in place, -1 on a bad index */
int oct_unet_debug_layer_fused(const oct_unet* h, int layer);

const char* oct_last_error(void);
/* "oct_unet_hip <ver> (gfx950) src:<12 hex digits>": the digits are the SHA-256 of the sources the library was built from
 * (csrc build.sh); the Python binding refuses a library whose stamp differs from the sources beside it */
const char* oct_version(void);

#ifdef __cplusplus
}
#endif
#endif /* OCT_UNET_H */
