/*
 * fosvos_hip.h - C ABI of libfosvos_hip.so: hand-written HIP (gfx950 / MI355X) kernels for the
 * OSVOS-VGG fine-tune hot path of klausondrag/FOSVOS.
 *
 * The reference has no FFI layer: its hot path runs through stock torch.nn modules
 * (src/networks/osvos_vgg.py:42-48,56,90-93 and src/layers/osvos_layers.py:17-54), i.e. the
 * arithmetic lives in third-party torch/cuDNN.  Each entry point below replaces one of those
 * call sites; the citation after "replaces:" names it (paths relative to the reference root).
 * The Python host (fosvos_amd/) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless stated otherwise;
 *   - the library allocates nothing persistent: outputs and workspaces belong to the caller,
 *     `*_workspace_bytes` tells how much scratch an op needs;
 *   - every call is asynchronous on `stream` (a hipStream_t) of `device`; no implicit sync;
 *   - return 0 on success, a negative FOSVOS_E_* code otherwise; fosvos_last_error() gives a
 *     thread-local message.  Nothing aborts or throws across the ABI;
 *   - re-entrant; the device is selected on every call (autograd runs backward on another thread);
 *   - no hidden state: the only objects that outlive a call are the inter-stream events of the multi-stream network
 *     calls, and those live in a caller-owned context (fosvos_ctx, one per model), never in the library.
 *
 * Tensor layouts
 *   frame   fp32 NCHW [N,3,H,W]                  (the reference's input layout)
 *   act     bf16 NHWC [N,H,W,C], C % 32 == 0     (internal feature maps, uint16_t storage)
 *   side    fp32 NHWC [N,h,w,16]                 (side_prep outputs)
 *   logit   fp32 [N,1,H,W]
 *   weight  fp32 OIHW [Co,Ci,3,3] masters as in the reference state_dict; bf16 packed copies
 *           [Ci/32][9][4][Co][8] for the MFMA kernels (see fosvos_pack_conv3x3_weights).
 */
#ifndef FOSVOS_HIP_H
#define FOSVOS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 33 also covers the entries added since without touching an existing symbol or struct (additive: an older caller sees no
 * difference): fosvos_conv3x3_fwd_pool_codes, fosvos_conv3x3_pool_codes_bytes, fosvos_maxpool2x2_ceil_bwd_codes,
 * fosvos_vgg_stage1_compact, fosvos_vgg_forward_flags, fosvos_vgg_forward_streams_flags, fosvos_vgg_backward_flags.
 * 34: no symbol or layout changed, but fosvos_resnet_net.first_unfused is now taken at its word (an older caller that
 * left it 0 for a wide or fp32 first layer sees a difference), and fosvos_resnet_arena_bytes shrank. */
#define FOSVOS_ABI_VERSION 34

#define FOSVOS_OK 0
#define FOSVOS_E_SHAPE (-1)     /* unsupported or inconsistent shape            */
#define FOSVOS_E_ARG (-2)       /* null pointer / bad flag                       */
#define FOSVOS_E_WORKSPACE (-3) /* caller workspace too small                    */
#define FOSVOS_E_HIP (-4)       /* HIP runtime error (message has the hip text)  */

/* conv epilogue flags */
#define FOSVOS_CONV_RELU 1u    /* y = max(y, 0)                                   */
#define FOSVOS_CONV_OUT_F32 2u /* store fp32 NHWC instead of bf16 NHWC            */
#define FOSVOS_CONV_FP32_MATH 4u /* fosvos_conv7x7s2_first_fwd only: fp32 frame and weights on the vector ALU */

int fosvos_abi_version(void);

/* ---- launch profiler --------------------------------------------------------------------------------------------
 * Between _start and _stop every kernel the library launches (from any entry point, the native layer loops
 * included) is bracketed by a pair of timing hipEvents recorded on the stream the kernel is launched on, so the
 * two-stream backward is measured as it ships.  _stop synchronises the device and returns one record per kernel name
 * (the names rocprofv3 --kernel-trace prints, templates included where several instantiations run): launches, summed
 * event time in ms, summed algorithmic FLOPs (0 for the byte movers).  The events are created by _start (room for
 * max_launches launches; later ones go untimed) and destroyed by _stop: the only allocation the library ever makes,
 * and only on request.  One profile at a time per process. */
typedef struct fosvos_profile_record {
    char name[96];
    int launches;
    double ms;
    double flops;
} fosvos_profile_record;
int fosvos_profile_start(int device, int max_launches);
int fosvos_profile_stop(int device, fosvos_profile_record *out, int capacity, int *n_out);
const char *fosvos_last_error(void);
/* Name of the gfx target the code object was built for ("gfx950"). */
const char *fosvos_build_arch(void);

/* ---- execution context ------------------------------------------------------------------------------------------
 * The multi-stream network calls (fosvos_vgg_forward_streams, fosvos_vgg_backward, fosvos_resnet_forward with an
 * aux_stream) order their streams with timing-disabled hipEvents, and fosvos_vgg_backward publishes its gradient
 * buckets through such events.  They belong to a context the CALLER creates, owns and destroys - one per model (or per
 * host thread that drives a model): two models trained from two host threads on one GPU never share an event, and
 * fosvos_vgg_grad_bucket_wait refers to the last backward pass OF ITS CONTEXT, not "of the device".  A context is bound
 * to one device; calls on one context must not overlap in time (one host thread at a time).  Nothing else in the
 * library keeps mutable state between calls (immutable per-device kernel attributes aside).
 * _destroy does not synchronise: the caller makes sure the streams are done with the events (as for any hipEvent). */
typedef struct fosvos_ctx fosvos_ctx;
int fosvos_ctx_create(int device, fosvos_ctx **ctx_out);
int fosvos_ctx_destroy(fosvos_ctx *ctx);
int fosvos_ctx_device(const fosvos_ctx *ctx); /* the device the context was created on, -1 for NULL */

/* ---- layout helpers (test/debug plumbing and the model's input/feature export) -------------- */
/* fp32 NCHW -> bf16 NHWC, channels zero-padded from C to Cpad (Cpad % 8 == 0, Cpad >= C). */
int fosvos_nchw_f32_to_nhwc_bf16(const float *src, uint16_t *dst, int N, int C, int H, int W, int Cpad,
                                 int device, void *stream);
/* bf16 NHWC (first C of Cpad channels) -> fp32 NCHW. */
int fosvos_nhwc_bf16_to_nchw_f32(const uint16_t *src, float *dst, int N, int C, int H, int W, int Cpad,
                                 int device, void *stream);
/* fp32 NHWC <-> fp32 NCHW */
int fosvos_nhwc_f32_to_nchw_f32(const float *src, float *dst, int N, int C, int H, int W, int device, void *stream);
int fosvos_nchw_f32_to_nhwc_f32(const float *src, float *dst, int N, int C, int H, int W, int device, void *stream);
/* Where fosvos_vgg_forward / _backward keep each tensor in their arena (test/debug plumbing: the layer-parity tests read
 * every layer back).  Byte offsets from the (256-byte aligned) arena base and unpadded byte sizes, from the same host
 * arithmetic the two calls use (no device call).  Regions: act[c] / gact[c] bf16 NHWC [N,h,w,Co_c] (conv c's output and the gradient wrt it),
 * pooled[s] / gpooled[s] bf16 NHWC [N,h,w,C] (the input of stage s+1 and its gradient), side[i] fp32 NHWC [N,h,w,16],
 * dside[i] bf16 NHWC [N,h,w,32] (channels 16..31 zero), bits0 [N,H,W,8] bytes (conv1_1's ReLU mask); then the op
 * workspaces: ws (main stream split-K), hws (head backward), wsa_conv[c] / wsa_side[i] (weight-gradient slabs).
 * stage_h / stage_w: the five stage resolutions.  The layout may change with any ABI version. */
typedef struct fosvos_vgg_arena_layout_info {
    size_t total; /* fosvos_vgg_arena_bytes */
    int stage_h[5], stage_w[5];
    size_t act[13], gact[13], act_bytes[13];
    size_t pooled[4], gpooled[4], pooled_bytes[4];
    size_t side[4], side_bytes[4];
    size_t dside[4], dside_bytes[4];
    size_t bits0, bits0_bytes;
    size_t ws, ws_bytes, hws, hws_bytes;
    size_t wsa_conv[13], wsa_conv_bytes[13], wsa_side[4], wsa_side_bytes[4];
} fosvos_vgg_arena_layout_info;
int fosvos_vgg_arena_layout(int N, int H, int W, fosvos_vgg_arena_layout_info *out);

/* ---- weight packing ---------------------------------------------------------------------------
 * fp32 OIHW master -> the two bf16 images the MFMA kernels read.
 *   w_fwd  [ceil(Ci/32)][9][4][Co_pad][8] : element (co,ci,tap) of the forward conv
 *   w_dgrad[ceil(Co/32)][9][4][Ci_pad][8] : element (ci,co,8-tap), i.e. the transposed, 180-degree
 *                                           rotated filter, so dgrad runs as a forward conv
 * Channel counts are zero-padded to multiples of 32 on the contraction side and to 16 on the
 * output side (Co_pad = roundup(Co,16), Ci_pad = roundup(Ci,16)).  Either output may be NULL.
 * replaces: the weight operand of nn.Conv2d (src/networks/osvos_vgg.py:42,92). */
int fosvos_pack_conv3x3_weights(const float *w_oihw, int Co, int Ci, uint16_t *w_fwd, uint16_t *w_dgrad,
                                int device, void *stream);
size_t fosvos_packed_weight_elems(int out_ch, int in_ch); /* elements of one packed image */

/* Both images of several layers in ONE launch (what the shipped module does after every optimizer step; replaces
 * 2 launches per layer).  Entry i packs w [Co,Ci,3,3] into w_fwd and/or w_dgrad (either may be NULL); Ci % 32 == 0.
 * `entries` is host memory, read before the call returns. */
typedef struct fosvos_pack_entry {
    const float *w;
    uint16_t *w_fwd, *w_dgrad;
    int Co, Ci;
} fosvos_pack_entry;
int fosvos_pack_conv3x3_weights_multi(const fosvos_pack_entry *entries, int n, int device, void *stream);

/* ---- first layer: conv1_1 (Ci = 3) straight from the fp32 NCHW frame --------------------------
 * y[N,H,W,Co] bf16 = relu(conv3x3(frame, w, pad 1) + b), fp32 VALU arithmetic (K = 27).
 * relu_bits [N,H,W,Co/8] bytes (NULL = none): the ReLU mask of y as one bit per element, bit e of byte g set where
 * y[..., 8 g + e] > 0 - what fosvos_conv3x3_dgrad_bits reads instead of y.
 * replaces: stages[0][0..1] = Conv2d(3,64,3,pad=1)+ReLU (src/networks/osvos_vgg.py:92-93). */
int fosvos_conv3x3_first_fwd(const float *frame, const float *w_oihw, const float *bias, uint16_t *y, uint8_t *relu_bits,
                             int N, int H, int W, int Co, int device, void *stream);
/* Launch geometry of the above: 8 x 32-pixel tiles and the (persistent) workgroups that walk them; tiles > workgroups
 * means every workgroup loops over several tiles with its double-buffered staging.  Host arithmetic only. */
int fosvos_conv3x3_first_plan(int N, int H, int W, int *tiles, int *workgroups);
/* dw[Co,3,3,3], db[Co] (fp32, overwritten) from the frame and dy[N,H,W,Co] bf16.  No dgrad: the
 * image needs no gradient.  workspace: fosvos_conv3x3_first_wgrad_workspace_bytes. */
int fosvos_conv3x3_first_wgrad(const float *frame, const uint16_t *dy, float *dw_oihw, float *dbias, int N, int H,
                               int W, int Co, void *workspace, size_t workspace_bytes, int device, void *stream);
size_t fosvos_conv3x3_first_wgrad_workspace_bytes(int N, int H, int W, int Co);

/* ---- 3x3 conv, pad 1, stride 1, as an implicit GEMM on bf16 MFMA with fp32 accumulation -------
 * y[N,H,W,Co] = epilogue( sum_{tap,ci} x[N,H+dy,W+dx,ci] * w[co,ci,tap] + bias[co] )
 *   x        bf16 NHWC with Ci_pad = roundup(Ci,32) channels
 *   w_packed the matching image from fosvos_pack_conv3x3_weights
 *   bias     fp32 [Co] or NULL
 *   y        bf16 NHWC with Co channels (Co % 16 == 0), or fp32 NHWC when FOSVOS_CONV_OUT_F32
 * replaces: Conv2d(3x3,pad=1)[+ReLU] in stages[*] and side_prep[*]
 *           (src/networks/osvos_vgg.py:42,92-93). */
int fosvos_conv3x3_fwd(const uint16_t *x, const uint16_t *w_packed, const float *bias, void *y, int N, int H, int W,
                       int Ci, int Co, unsigned flags, void *workspace, size_t workspace_bytes, int device,
                       void *stream);

/* Stride 2 (pad 1): y[N,(H-1)/2+1,(W-1)/2+1,Co] = act(conv3x3(x) + bias) at the even pixels.  Computed by the
 * stride-1 MFMA kernel with a subsampling store: 4x the arithmetic of a strided kernel, which the MFMA rate more than pays
 * for at Ci >= 32.  Co % 64 == 0 or Co = 32; one launch, the workspace is not used.
 * replaces: the stride-2 conv1 + bn1 + relu that opens ResNet stages 2-4 (src/networks/osvos_resnet.py:101-103). */
int fosvos_conv3x3_s2_fwd(const uint16_t *x, const uint16_t *w_packed, const float *bias, uint16_t *y, int N, int H, int W,
                          int Ci, int Co, unsigned flags, void *workspace, size_t workspace_bytes, int device, void *stream);
/* The residual form: y = act(conv3x3(x) + bias + addend), ReLU (FOSVOS_CONV_RELU) applied AFTER the add; addend is bf16
 * [N,H,W,Co] or NULL.  Co % 64 == 0 or Co = 32; without an addend also Co = 16, then optionally FOSVOS_CONV_OUT_F32 (the
 * side_prep form).  Always ONE launch (no split-K, the workspace is not used): this is the inference
 * form, whose chain of small dependent launches pays more for a second kernel than the split wins.
 * replaces: conv2 + bn2 + `out += residual` + relu of torchvision's BasicBlock (src/networks/osvos_resnet.py:203-214). */
int fosvos_conv3x3_fwd_add(const uint16_t *x, const uint16_t *w_packed, const float *bias, const uint16_t *addend,
                           void *y, int N, int H, int W, int Ci, int Co, unsigned flags, void *workspace,
                           size_t workspace_bytes, int device, void *stream);
/* fosvos_conv3x3_fwd plus MaxPool2d(2,2,ceil_mode=True) of its output in the same launch (the last conv of a VGG stage
 * feeds both the side branch and the pool, src/networks/osvos_vgg.py:90-93): y as above (bf16, Co % 64 == 0),
 * y_pool = [N, ceil(H/2), ceil(W/2), Co] bf16.  Saves the pool kernel's re-read of y. */
int fosvos_conv3x3_fwd_pool(const uint16_t *x, const uint16_t *w_packed, const float *bias, uint16_t *y,
                            uint16_t *y_pool, int N, int H, int W, int Ci, int Co, unsigned flags, void *workspace,
                            size_t workspace_bytes, int device, void *stream);
/* The pooled forward form WITHOUT the dense output, for a layer whose output only the pool's backward would read (conv1_2
 * of a training pass: 52 MB a 480x854 frame): y_pool as fosvos_conv3x3_fwd_pool writes it, bit for bit, and the pool's WINNER
 * CODES, codes[N, ceil(H/2), ceil(W/2), Co/8] 32-bit words (fosvos_conv3x3_pool_codes_bytes of them).  The word of a pooled
 * pixel and channel group holds one 4-bit one-hot nibble per channel: channel 8 g + 2 i + h at bit 4 i + 16 h (i = 0..3,
 * h = 0, 1).  Window pixels are numbered k = 2 dy + dx in scan order; bit k is set iff pixel k is the first maximum in scan
 * order (a later pixel wins only with a strictly larger value; pixels outside the image never win) AND that maximum is > 0.
 * A zero nibble: the ReLU output is 0 in the whole window, the gradient goes nowhere.  For finite activations that is what
 * fosvos_maxpool2x2_ceil_bwd (relu_mask = 1) derives from the dense output; a NaN activation wins like the largest value,
 * as it does in the pooled map.  flags must be FOSVOS_CONV_RELU.  Only the persistent kernel has this form: a shape it does
 * not take (fosvos_conv3x3_fwd_plan(..).persistent == 0 for the same shape and flags) is FOSVOS_E_SHAPE. */
int fosvos_conv3x3_fwd_pool_codes(const uint16_t *x, const uint16_t *w_packed, const float *bias, uint16_t *y_pool,
                                  uint32_t *codes, int N, int H, int W, int Ci, int Co, unsigned flags, int device,
                                  void *stream);
size_t fosvos_conv3x3_pool_codes_bytes(int N, int H, int W, int C); /* 0 for a bad shape (C % 8 != 0) */
/* Scratch for fwd/dgrad with `in_ch` contraction and `out_ch` output channels (split-K partial
 * slabs for layers whose pixel count alone cannot fill 256 CUs; 0 when none is needed). */
size_t fosvos_conv3x3_workspace_bytes(int N, int H, int W, int in_ch, int out_ch);
/* Which kernel instantiation fosvos_conv3x3_fwd / _fwd_pool / _dgrad launch for a shape (`in_ch` contraction, `out_ch`
 * output channels): the pixel tile (tile_h x tile_w) x tile_co output channels of one workgroup, the K split count and the
 * number of workgroups.  Pure host arithmetic (no device call); the parity tests use it to assert that the cases they run
 * really select the instantiations the 480x854 step runs (k_conv3x3_igemm<Tile<tile_h, tile_w, tile_co, ..>>). */
typedef struct fosvos_conv3x3_plan_info {
    int tile_h, tile_w, tile_co;
    int k_splits;
    int workgroups; /* per K split */
    int persistent; /* 1: the persistent eight-wave forward kernel k_conv3x3_pp (conv_pp.hip): `workgroups` of them, one per
                     * CU, walk the 8 x 32-pixel x 64-channel tiles in two groups of four waves that alternate between the
                     * MFMAs of a K chunk and the memory work of the other tile */
} fosvos_conv3x3_plan_info;
int fosvos_conv3x3_plan(int N, int H, int W, int in_ch, int out_ch, fosvos_conv3x3_plan_info *out);
/* The same question for a FORWARD launch (fosvos_conv3x3_fwd / _fwd_pool with these flags): bf16-output launches whose
 * tiles fill the chip run the persistent kernel; every other form (data gradient, residual add, stride 2, fp32 output) is
 * what fosvos_conv3x3_plan reports. */
int fosvos_conv3x3_fwd_plan(int N, int H, int W, int in_ch, int out_ch, unsigned flags, fosvos_conv3x3_plan_info *out);
/* dx = mask( dgrad(dy) ) + addend:  the same kernel run on the rotated/transposed filter image.
 *   dy       bf16 NHWC, Co_pad = roundup(Co,32) channels (Co = the forward op's OUTPUT channels)
 *   relu_src bf16 NHWC [N,H,W,Ci] or NULL: where relu_src <= 0 the computed gradient is zeroed
 *            (ReLU backward of the layer that produced x, fused)
 *   addend   bf16 NHWC [N,H,W,Ci] or NULL: added after masking (gradient arriving at the same
 *            tensor through another consumer); may alias dx
 * replaces: autograd's conv backward-data for the same modules. */
int fosvos_conv3x3_dgrad(const uint16_t *dy, const uint16_t *w_dgrad_packed, const uint16_t *relu_src,
                         const uint16_t *addend, uint16_t *dx, int N, int H, int W, int Ci, int Co, void *workspace,
                         size_t workspace_bytes, int device, void *stream);
/* The same with the ReLU mask given as ONE BIT per element: relu_bits [N,H,W,Ci/8] bytes, bit e of byte g set where channel
 * 8 g + e of the producing layer's output is > 0 (fosvos_conv3x3_first_fwd writes it for conv1_1).  Bit for bit the
 * result of fosvos_conv3x3_dgrad on the bf16 image the bits were taken from; 1/16 of the mask bytes - conv1_2's data gradient
 * at 480x854 is bound by HBM traffic. */
int fosvos_conv3x3_dgrad_bits(const uint16_t *dy, const uint16_t *w_dgrad_packed, const uint8_t *relu_bits,
                              const uint16_t *addend, uint16_t *dx, int N, int H, int W, int Ci, int Co, void *workspace,
                              size_t workspace_bytes, int device, void *stream);
/* Data gradient of a conv whose INPUT x also feeds a MaxPool2d(2, 2, ceil_mode=True) - side_prep[i] on a stage output
 * (src/networks/osvos_vgg.py:61-83: `side_prep[i](x)` beside `stages[i+1](x)`) - with the pool's backward in the same pass:
 *   dx = [x > 0] * dgrad(dy) + maxpool2x2_ceil_bwd(x, d_pooled)         (fosvos_maxpool2x2_ceil_bwd with relu_mask = 1)
 *   x        bf16 NHWC [N,H,W,Ci]: the post-ReLU stage output (ReLU mask and the pool's arg-max source)
 *   d_pooled bf16 NHWC [N,ceil(H/2),ceil(W/2),Ci]: gradient wrt the pooled map
 * Bit for bit the result of the pool backward followed by fosvos_conv3x3_dgrad(dy, w, x, addend = that, dx), which is also
 * what runs for shapes whose plan has no fused form (split-K launches, Ci not a multiple of 64).  dx must not alias x.
 * replaces: autograd's backward of the two consumers of a stage output. */
int fosvos_conv3x3_dgrad_unpool(const uint16_t *dy, const uint16_t *w_dgrad_packed, const uint16_t *x,
                                const uint16_t *d_pooled, uint16_t *dx, int N, int H, int W, int Ci, int Co,
                                void *workspace, size_t workspace_bytes, int device, void *stream);
/* dw[Co,Ci,3,3] (fp32 OIHW) and db[Co] (may be NULL) from x[N,H,W,Ci] and dy[N,H,W,Co_pad] (bf16).
 * Deterministic: split partial sums are written as slabs to the workspace and reduced in a fixed
 * order.  accumulate != 0 adds into dw/db instead of overwriting.
 * replaces: autograd's conv backward-weight/bias. */
int fosvos_conv3x3_wgrad(const uint16_t *x, const uint16_t *dy, float *dw_oihw, float *dbias, int N, int H, int W,
                         int Ci, int Co, int accumulate, void *workspace, size_t workspace_bytes, int device,
                         void *stream);
size_t fosvos_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int Ci, int Co);
/* The two halves of fosvos_conv3x3_wgrad, for callers that batch or time them apart (the network call queues every
 * layer's reduction and runs them together): _slabs runs the MFMA kernel, leaving per-split partial sums (and, with
 * with_bias != 0, bias partials) in the workspace; _reduce turns that workspace into dw / db (db NULL = no bias). */
int fosvos_conv3x3_wgrad_slabs(const uint16_t *x, const uint16_t *dy, int with_bias, int N, int H, int W, int Ci, int Co,
                               void *workspace, size_t workspace_bytes, int device, void *stream);
int fosvos_conv3x3_wgrad_reduce(float *dw_oihw, float *dbias, int N, int H, int W, int Ci, int Co, int accumulate,
                                void *workspace, size_t workspace_bytes, int device, void *stream);

/* ---- 2x2 stride-2 ceil-mode max pool on bf16 NHWC ---------------------------------------------
 * y[N,ceil(H/2),ceil(W/2),C]; ragged last row/column windows hold 2 or 1 elements.
 * replaces: MaxPool2d(2,2,ceil_mode=True) (src/networks/osvos_vgg.py:90). */
int fosvos_maxpool2x2_ceil_fwd(const uint16_t *x, uint16_t *y, int N, int H, int W, int C, int device, void *stream);
/* dx[N,H,W,C]: dy routed to the first maximum of each window in (row, column) scan order, zero
 * elsewhere; relu_mask != 0 also zeroes it where x <= 0 (ReLU backward of the producer, fused). */
int fosvos_maxpool2x2_ceil_bwd(const uint16_t *x, const uint16_t *dy, uint16_t *dx, int N, int H, int W, int C,
                               int relu_mask, int device, void *stream);
/* The same dx (relu_mask = 1) from the winner codes fosvos_conv3x3_fwd_pool_codes wrote for x, without x: bit for bit
 * fosvos_maxpool2x2_ceil_bwd(x, dy, dx, .., 1) for finite x.  20 bytes read per pooled pixel and 8 channels instead of 80. */
int fosvos_maxpool2x2_ceil_bwd_codes(const uint32_t *codes, const uint16_t *dy, uint16_t *dx, int N, int H, int W, int C,
                                     int device, void *stream);

/* ---- fused side-output head -------------------------------------------------------------------
 * For the four scales s (stride f = 2,4,8,16; deconv kernel k = 2f) with side[s] fp32 NHWC
 * [N,hs[s],ws[s],16]:
 *   fused[n,0,Y,X]   = fuse_b + sum_s sum_c fuse_w[16 s + c] * crop(up_s(side[s]))[c,Y,X]
 *   side_out[s][..]  = crop(up1_s(dsn_b[s] + sum_c dsn_w[s][c] * side[s][c]))        (optional)
 * up_s is the transposed conv with the DIAGONAL of upscale[s].weight, passed channel-fastest as
 * filt[s] = [k][k][16] fp32 (one k x k filter per channel); up1_s uses filt1[s] = [k][k].  crop is the
 * reference's centre crop (floor(d/2) leading pixels removed).
 * filt_uniform: bit s set = the caller PROMISES that the 16 channel filters of filt[s] are identical, element for element
 * (what interp_surgery writes - src/layers/osvos_layers.py:70-81 - and the optimizers keep: lr 0,
 * src/util/network_provider.py:110-111,154-155).  The kernels then contract the channels once per low-resolution pixel
 * and apply ONE k x k filter (same sums in another order; 16x fewer multiply-adds and LDS reads).  0 = the general form.
 * A set bit with filters that differ between channels evaluates channel 0's filter for all: the check is the caller's.
 * replaces: upscale[s], upscale_[s], score_dsn[s], center_crop, torch.cat and fuse
 *           (src/networks/osvos_vgg.py:69-82, src/layers/osvos_layers.py:47-54). */
int fosvos_head_fwd(const float *const side[4], const int hs[4], const int ws[4], const float *const filt[4],
                    const float *const filt1[4], const float *dsn_w /*[4][16]*/, const float *dsn_b /*[4]*/,
                    const float *fuse_w /*[64]*/, const float *fuse_b /*[1]*/, float *fused,
                    float *const side_out[4] /* all NULL or all set */, int N, int H, int W, int filt_uniform, int device,
                    void *stream);
/* Backward of the above.
 *   d_fused [N,1,H,W] fp32 or NULL;  d_side_out[s] [N,1,H,W] fp32 or NULL (all or none)
 *   d_side[s]   bf16 NHWC [N,hs,ws,32]: channels 0..15 = gradient wrt side[s], 16..31 = 0 (the
 *               padded image the side_prep dgrad/wgrad MFMA kernels read)
 *   d_fuse_w[64], d_fuse_b[1], d_dsn_w[4*16], d_dsn_b[4]: fp32, overwritten (d_dsn_* may be NULL
 *               when d_side_out is NULL).
 * workspace: fosvos_head_bwd_workspace_bytes. */
int fosvos_head_bwd(const float *const side[4], const int hs[4], const int ws[4], const float *const filt[4],
                    const float *const filt1[4], const float *dsn_w, const float *fuse_w, const float *d_fused,
                    const float *const d_side_out[4], uint16_t *const d_side[4], float *d_fuse_w, float *d_fuse_b,
                    float *d_dsn_w, float *d_dsn_b, int N, int H, int W, int filt_uniform /* as fosvos_head_fwd */,
                    void *workspace, size_t workspace_bytes, int device, void *stream);
size_t fosvos_head_bwd_workspace_bytes(int N, int H, int W);

/* ---- class-balanced BCE-with-logits, loss and gradient in one call ----------------------------
 * y_i = label_i >= 0.5; Np = #y, Nn = numel - Np;
 * loss = (Nn/numel) * sum_{y=1} l_i + (Np/numel) * sum_{y=0} l_i,  l_i = max(x,0) - x y + log(1+exp(-|x|))
 * [divided by numel when size_average]; grad_i = scale * w_i * (sigmoid(x_i) - y_i) with the same
 * weights (and the 1/numel factor when size_average).  Reductions run over the whole batch tensor
 * and are deterministic (fixed-order fp64 partials).  loss_out: one fp32 on the device.
 * grad may be NULL.  workspace: fosvos_cbce_workspace_bytes.
 * Every entry point of this block runs the same three kernels (count, loss, finish) through one host path, which makes all
 * its argument checks before the first launch: logits, label and grad 16-byte aligned, the workspace 8-byte aligned (device
 * allocations are; a single-map call with a workspace off an 8-byte boundary was never valid and is now refused) and large
 * enough.  The loss kernel is one template over the number of logit maps that share a label batch, so the forms below agree
 * bit for bit by construction.
 * replaces: class_balanced_cross_entropy_loss + its autograd (src/layers/osvos_layers.py:17-44). */
int fosvos_cbce_loss(const float *logits, const float *label, int64_t numel, int size_average, float grad_scale,
                     float *loss_out, float *grad, void *workspace, size_t workspace_bytes, int device,
                     void *stream);
size_t fosvos_cbce_workspace_bytes(int64_t numel);
/* The loss of EVERY FRAME of a batch separately, in one set of launches: logits / label / grad are [n_frames][frame_numel],
 * loss_out gets n_frames values, each what fosvos_cbce_loss returns for that frame alone (own class counts).  The online
 * loop uses it when it runs several micro-batches of an accumulation cycle as one batched pass: the reference computes
 * the loss per frame (src/train_online.py:80 on a [1,1,H,W] tensor).  frame_numel must be a multiple of 4 when
 * n_frames > 1; workspace: n_frames x fosvos_cbce_workspace_bytes. */
int fosvos_cbce_loss_frames(const float *logits, const float *label, int64_t frame_numel, int n_frames, int size_average,
                            float grad_scale, float *loss_out, float *grad, void *workspace, size_t workspace_bytes,
                            int device, void *stream);
/* fosvos_cbce_loss_frames in its three launches, for a caller that has other work to put between them (the online loop):
 * FOSVOS_CBCE_COUNT needs only the labels (it can run before the forward pass that produces the logits), FOSVOS_CBCE_LOSS
 * writes grad and the loss partials (the backward pass needs nothing more), FOSVOS_CBCE_FINISH writes loss_out (it can run
 * behind the backward pass).  `parts` = the stages of this call, run in that order; arguments a stage does not read may
 * be NULL (COUNT: logits, loss_out, grad; FINISH: logits, label, grad).  The stages of one loss share `workspace`: same
 * pointer, untouched by anything else in between.  All three in one call = fosvos_cbce_loss_frames, bit for bit. */
#define FOSVOS_CBCE_COUNT 1
#define FOSVOS_CBCE_LOSS 2
#define FOSVOS_CBCE_FINISH 4
int fosvos_cbce_loss_frames_parts(const float *logits, const float *label, int64_t frame_numel, int n_frames,
                                  int size_average, float grad_scale, float *loss_out, float *grad, void *workspace,
                                  size_t workspace_bytes, int parts, int device, void *stream);
/* The per-frame loss of n_maps LOGIT MAPS THAT SHARE ONE LABEL BATCH (the offline objective: four side maps and the fused
 * map per frame, src/train_offline.py:85-91), with the stages of the call above.  logits / grad: HOST arrays of n_maps
 * device pointers, each [n_frames][frame_numel] (separate tensors; grad, or any entry of it, may be NULL); map_scale: n_maps
 * HOST floats, map m's gradient is multiplied by map_scale[m]; loss_out: [n_frames][n_maps] UNWEIGHTED loss values.  One
 * count per frame serves all maps and one launch writes every gradient: a thread reads its labels once and walks the maps
 * (4 + n_maps x 8 bytes per pixel against n_maps x 16).  For every frame and map the result equals fosvos_cbce_loss_frames
 * on that map with grad_scale = map_scale[m], bit for bit (that call is this one with n_maps = 1).  1 <= n_maps <= FOSVOS_CBCE_MAX_MAPS; frame_numel a multiple of 4
 * when n_frames > 1; workspace: fosvos_cbce_multi_workspace_bytes, shared by the stages of one loss.  Arguments a stage does
 * not read may be NULL (COUNT: logits, map_scale, loss_out, grad; FINISH: logits, label, map_scale, grad). */
#define FOSVOS_CBCE_MAX_MAPS 8
size_t fosvos_cbce_multi_workspace_bytes(int64_t frame_numel, int n_frames, int n_maps);
int fosvos_cbce_loss_frames_multi(const float *const *logits, const float *label, int64_t frame_numel, int n_frames,
                                  int n_maps, int size_average, const float *map_scale, float *loss_out, float *const *grad,
                                  void *workspace, size_t workspace_bytes, int parts, int device, void *stream);
/* The same loss on ONE SHARD of a batch that is split over data-parallel ranks.  The reference counts positives /
 * negatives over the whole batch tensor (src/layers/osvos_layers.py:28-39), so the class weights of a shard must
 * come from the whole batch: batch_counts = DEVICE double[2] {positives, pixels} summed over all shards (the caller
 * all-reduces them).  loss_out is this shard's part of the batch loss (the parts add up to it); with size_average the
 * division is by the batch's pixel count.  grad is what the single-process batch would hold for these pixels. */
int fosvos_cbce_loss_batch_counts(const float *logits, const float *label, int64_t numel, int size_average,
                                  float grad_scale, const double *batch_counts, float *loss_out, float *grad,
                                  void *workspace, size_t workspace_bytes, int device, void *stream);
/* The per-frame loss WITH IGNORED PIXELS (online adaptation trains on pseudo-labels that leave most of a frame undecided):
 * void_px uint8 [n_frames][frame_numel], non-zero = ignored.  Np and Nn are counted over the valid pixels only and
 * Ntot = Np + Nn takes numel's place: loss = (Nn/Ntot) * sum_{valid, y=1} l_i + (Np/Ntot) * sum_{valid, y=0} l_i [divided by
 * Ntot when size_average]; grad_i = scale * w_i * (sigmoid(x_i) - y_i) on a valid pixel and exactly +0.0 on a void one, whose
 * logit - a NaN too - reaches neither a sum nor a gradient.  Ntot == 0: loss 0, gradient 0.  util/online_adapt.cbce_void
 * states it in float64.  (Not upstream OSVOS-PyTorch's void_pixels variant, which still counts void pixels as negatives.)
 * The same kernels as fosvos_cbce_loss_frames in a compile-time void form, the same fixed-order sums: with void_px all zero
 * the results are that call's bit for bit, a frame of a batch equals the frame alone, two calls agree.  void_px 4-byte
 * aligned, everything else as for fosvos_cbce_loss_frames; workspace: fosvos_cbce_void_workspace_bytes. */
size_t fosvos_cbce_void_workspace_bytes(int64_t frame_numel, int n_frames);
int fosvos_cbce_loss_frames_void(const float *logits, const float *label, const uint8_t *void_px, int64_t frame_numel,
                                 int n_frames, int size_average, float grad_scale, float *loss_out, float *grad,
                                 void *workspace, size_t workspace_bytes, int device, void *stream);

/* ---- SGD with momentum, torch.optim.SGD semantics, many tensors per launch --------------------
 * For tensor t with n[t] elements: g = grad + wd[t]*p; buf = first_step ? g : momentum*buf + g;
 * p -= lr[t]*buf.  `table` is a DEVICE array of n_tensors fosvos_sgd_entry records.
 * `first_step` is a flag word: bit 0 = first step (buf = g), bit 1 (FOSVOS_SGD_ZERO_GRAD) = every gradient is overwritten
 * with zeros once it has been read - optimizer.step() + optimizer.zero_grad() (src/train_online.py:100-104) in one pass over
 * the gradients instead of a step and a memset.
 * replaces: optim.SGD.step for the groups of src/util/network_provider.py:144-159 / 98-125. */
#define FOSVOS_SGD_FIRST_STEP 1
#define FOSVOS_SGD_ZERO_GRAD 2
typedef struct fosvos_sgd_entry {
    float *param;
    const float *grad; /* written (zeroed) only under FOSVOS_SGD_ZERO_GRAD */
    float *momentum_buf;
    int64_t numel;
    float lr;
    float weight_decay;
} fosvos_sgd_entry;
int fosvos_sgd_momentum_step(const fosvos_sgd_entry *table, int n_tensors, int64_t max_numel, float momentum,
                             int first_step, int device, void *stream);

/* ---- training-sample augmentation (offline training set resident on the device) -------------------------------
 * One training sample of DAVIS2016 -> the minibatch the reference's training loader yields for it (flip, then rescale:
 * src/util/io_helper.py:62-70, src/dataloaders/custom_transforms.py:63-111), in one launch on `stream`.
 *   frame     uint8 [H,W,3] (BGR, as decoded); mask uint8 [H,W]
 *   flip      nonzero: mirror left-right before the rescale
 *   col_taps / col_w  int32 / fp32 [OW][4]: clipped source columns and bicubic weights of each output column (16-byte
 *             aligned); row_taps / row_w [OH][4]: the same for the rows; col_near [OW], row_near [OH]: the mask's
 *             nearest-neighbour source column / row.  Indices refer to the (flipped) frame, as the host's resize computes
 *             them.  All six NULL: a plain copy (scale 1; OH == H and OW == W).
 *   img_lut   fp32 [256][3]: the image value of byte v in channel c (v - mean[c]); gt_lut fp32 [256]: the gt value of v
 *   image     fp32 [3,OH,OW] out; gt fp32 [OH,OW] out
 * Each output value is ((((0 + a0*w0) + a1*w1) + a2*w2) + a3*w3) in fp32 with every product rounded (no multiply-add
 * contraction), horizontally first and then vertically over the fp32 horizontal results: the numpy restatement of
 * cv2.resize in the training pipeline, bit for bit.  W <= 4096.
 * replaces: the per-iteration DataLoader worker's transforms of src/util/io_helper.py:62-70. */
int fosvos_augment_sample(const uint8_t *frame, const uint8_t *mask, int H, int W, int flip, const int32_t *col_taps,
                          const float *col_w, const int32_t *row_taps, const float *row_w, const int32_t *col_near,
                          const int32_t *row_near, int OH, int OW, const float *img_lut, const float *gt_lut, float *image,
                          float *gt, int device, void *stream);
/* fosvos_warp_sample: the same sample rotated and zoomed about its centre (flip, then the reference's ScaleNRotate,
 * src/dataloaders/custom_transforms.py:7-60: cv2.warpAffine at the frame's own size, bicubic for the frame, nearest for
 * the mask, 0 outside the source), bit for bit dataloaders/custom_transforms.warp_affine.
 *   frame, mask, flip, img_lut, gt_lut   as above, at any byte alignment; image fp32 [3,H,W] out; gt fp32 [H,W] out
 *   i00 .. i12   the INVERSE 2x3 matrix (destination -> source) in fp64: sx = (i00*x + i01*y) + i02, sy = (i10*x + i11*y)
 *                + i12, no contraction.  Mask: rint (half to even) of both, the table value of the byte there or 0.  Frame:
 *                floor of both, the fractions as fp32, interpolateCubic's weights (A = -0.75) in fp32, the 16 taps row-outer
 *                and column-inner as out = out + val * (wy[j] * wx[i]) from +0.0, val = 0 for a tap outside the source.
 *   renormalize  nonzero: the reference's `if min < 0: image -= min; if max > 1: image /= max` over the whole image in fp32
 *                (the gt is left alone: table values in [0, 1] make both steps no-ops).  The warp launch writes one (min, max)
 *                pair per workgroup to `workspace` (fosvos_warp_workspace_bytes(H, W) bytes, 4-byte aligned) and a second
 *                launch reduces all pairs in every workgroup and rewrites the image.  Finite table values only.
 *                Zero: one launch, no workspace (NULL, 0).
 * Refused: H or W above 8192, a non-finite coefficient, a matrix that sends one of the four output corners beyond +-2^30
 * (within that bound every source coordinate fits int32), renormalize without its workspace.  Every tap is bounds-checked.
 * replaces: the per-iteration DataLoader worker's ScaleNRotate, commented out in src/util/io_helper.py:62-70. */
int fosvos_warp_sample(const uint8_t *frame, const uint8_t *mask, int H, int W, int flip, double i00, double i01, double i02,
                       double i10, double i11, double i12, const float *img_lut, const float *gt_lut, float *image,
                       float *gt, int renormalize, void *workspace, size_t workspace_bytes, int device, void *stream);
size_t fosvos_warp_workspace_bytes(int H, int W); /* 0 for sizes fosvos_warp_sample refuses */
/* fosvos_lucid_sample: the same sample with the object moved against its background (opt-in; csrc/lucid.hip), bit for bit
 * dataloaders/lucid.py: compose.  ONE launch on `stream`; no workspace, no atomics, no workgroup waits for another.
 *   frame, background  u8 [H,W,3] (background: the frame with the object painted out, lucid.fill_background); mask u8 [H,W];
 *                all three at any byte alignment, mirrored first if `flip`
 *   b00 .. b12   the INVERSE 2x3 matrix of the background (destination -> source) in fp64, f00 .. f12 that of the object;
 *                coordinates as in fosvos_warp_sample.  fg_on == 0: no object - alpha = 0 and gt = 0 everywhere, and frame, mask
 *                and f00 .. f12 are not read
 *   gt           nearest (rint, half to even) through the object's matrix, the table value of the mask byte there or 0
 *   alpha        the four bilinear taps of `mask != 0` through the object's matrix (fractions and weights 1 - f, f in fp32,
 *                row-outer / column-inner, acc = acc + val * (wy[j] * wx[i]) from +0.0, 0 outside); exactly 1 where all four
 *                taps lie inside the frame and on the object
 *   image        B where alpha == 0, Fg where alpha == 1, else B + alpha * (Fg - B), each operation rounded in fp32; then
 *                * gain[c] + bias[c] (two roundings).  B / Fg: fosvos_warp_sample's bicubic gather of background / frame under
 *                its matrix; B is gathered only where alpha != 1, Fg only where alpha != 0.  image fp32 [3,H,W], gt fp32 [H,W]
 * Refused: H or W above 8192, a non-finite coefficient, gain or bias, a matrix that sends one of the four output corners
 * beyond +-2^30.  Every tap's address is clamped into the frame before the load. */
int fosvos_lucid_sample(const uint8_t *frame, const uint8_t *background, const uint8_t *mask, int H, int W, int flip, double b00,
                        double b01, double b02, double b10, double b11, double b12, double f00, double f01, double f02,
                        double f10, double f11, double f12, int fg_on, float gain0, float gain1, float gain2, float bias0,
                        float bias1, float bias2, const float *img_lut, const float *gt_lut, float *image, float *gt, int device,
                        void *stream);

/* ---- scoring a segmented sequence (DAVIS 2016 J and F) and its PNG bytes ------------------------------------------
 * The reference writes probability PNGs and leaves the measures to an outside toolkit (src/eval/README.md); these two
 * ops keep both on the device beside the logits.  The definitions are stated in numpy in util/davis_measures.py.
 *
 * fosvos_prob_bytes: logits fp32 [N,1,H,W] -> out uint8 [N,H,W], per frame bytescale(sigmoid(logits)) of
 * src/util/experiment_helper.py:57-64 evaluated in fp64: p = 1 / (1 + exp(-(double)x)), cmin / cmax = p at the frame's
 * smallest / largest logit, cscale = cmax - cmin (1 if that is 0), byte = (uint8)(clip((p - cmin) * (255 / cscale), 0,
 * 255) + 0.5).  minmax: fp32 [N,2] scratch of the caller (it holds each frame's {min, max} logit afterwards).  NaN-free
 * logits only.  Three launches on `stream`: 4 B read twice and 1 B written per pixel.
 * replaces: the host's sigmoid + scipy.misc.imsave stretch of src/util/experiment_helper.py:57-64. */
int fosvos_prob_bytes(const float *logits, int N, int H, int W, float *minmax, uint8_t *out, int device, void *stream);
/* fosvos_jf_counts: logits fp32 [N,1,H,W] and gt uint8 [N,H,W] (non-zero = object) -> counts int32 [N,6] per frame:
 * {inter, union, n_pred_b, n_gt_b, match_pred, match_gt} for the predicted mask A = (logit >= 0) and the ground truth
 * B = (gt != 0): |A and B|, |A or B|, |bmap(A)|, |bmap(B)|, |bmap(A) and dil(bmap(B), radius)|, |bmap(B) and
 * dil(bmap(A), radius)|.  bmap(S) at (y,x): S differs from its right, lower or lower-right neighbour (last row: right
 * only; last column: lower only; the corner: 0).  dil(M, r): M dilated by the disk dy*dy + dx*dx <= r*r, pixels outside
 * the image count as 0.  1 <= radius <= 63.  The op zeroes the counters itself; what `counts` and the workspace
 * (fosvos_jf_workspace_bytes, 8-byte aligned: two bit planes of [N][H][ceil(W/64)] 64-bit words) held before does not
 * matter.  Integer sums only: the result does not depend on the order the workgroups finish in.  Two launches. */
size_t fosvos_jf_workspace_bytes(int N, int H, int W);
int fosvos_jf_counts(const float *logits, const uint8_t *gt, int N, int H, int W, int radius, int32_t *counts,
                     void *workspace, size_t workspace_bytes, int device, void *stream);

/* ---- the probability PNGs, encoded on the device ------------------------------------------------------------------
 * fosvos_png_encode: bytes uint8 [N,H,W] (what fosvos_prob_bytes writes) -> N standalone 8-bit greyscale PNG files: frame n's
 * file is out[n * capacity .. n * capacity + lengths[n]), the bytes behind it are left as they were.  The layout is stated
 * in numpy in util/png_layout.py (the tests compare byte for byte): the filtered stream (filter None) is cut into segments
 * of 4096 bytes, each in an IDAT chunk of its own; a last IDAT holds the final block and the Adler-32.  huffman = 0 (fixed):
 * a segment is one fixed-Huffman deflate block (runs of a byte as distance-1 matches, everything else literals) closed by
 * an empty stored block - or a stored block where that is shorter.  huffman = 1 (fitted) adds a third form: a
 * dynamic-Huffman block (BTYPE = 10) whose literal/length code is fitted to the segment's tokens - deterministic two-queue
 * Huffman construction over the symbols sorted by (count, symbol), lengths limited to 15 bits by halving the counts,
 * canonical codes; HDIST = 0 (a match's distance costs 1 bit); a fixed, complete code-length code with HCLEN = 19; zero
 * runs of the length sequence as symbols 17 / 18.  Each segment takes the shortest of {fitted, fixed, stored}, fixed or
 * stored on a tie, so no file is longer than with huffman = 0.  Any other huffman: FOSVOS_E_ARG.  Any PNG reader decodes
 * the files to the input bytes; they are larger than a level-6 zlib stream of the same image.
 *   capacity   bytes reserved per frame in `out`, >= fosvos_png_capacity_bytes (the layout's size bound
 *              65 + H (W+1) + 17 ceil(H (W+1) / 4096): no image encodes to more, with either huffman)
 *   lengths    int32 [N]
 *   workspace  fosvos_png_workspace_bytes (16 B a segment, and with huffman != 0 288 B of code lengths more), 4-byte
 *              aligned; what it and `out` held before does not matter
 * H (W+1) <= 2^30.  Integer arithmetic only; two launches on `stream`.
 * replaces: the PIL encoder behind scipy.misc.imsave of src/util/experiment_helper.py:64. */
size_t fosvos_png_capacity_bytes(int N, int H, int W); /* per frame */
size_t fosvos_png_workspace_bytes(int N, int H, int W, int huffman);
int fosvos_png_encode(const uint8_t *bytes, int N, int H, int W, int huffman, uint8_t *out, size_t capacity, int32_t *lengths,
                      void *workspace, size_t workspace_bytes, int device, void *stream);

/* ---- several objects a sequence: label merge, per-object counts, palette files (ABI 31) ---------------------------------
 * One net per object is fine-tuned on "this object against everything else"; all K nets run on every frame.  The
 * definitions are stated in numpy in util/object_merge.py and util/png_layout.py (encode_indexed); the tests compare byte
 * for byte.
 *
 * fosvos_merge_objects: logits[k] fp32 [N,1,H,W] of net k (k = 0..K-1, 1 <= K <= FOSVOS_MAX_OBJECTS; `logits` is a host
 * array of K device pointers, which travel to the kernel by value) -> labels uint8 [N,H,W]: 0 where no logit of the pixel is
 * >= 0 (a NaN never is, -0.0 is), else 1 + k* with k* the lowest k among those holding the largest such logit.  For K = 1
 * that is the mask of fosvos_jf_counts.  One launch; 4 K B read and 1 B written per pixel.
 *
 * fosvos_jf_counts_labels: pred and gt uint8 [N,H,W] label maps -> counts int32 [N,K,6]: row (n, k-1) is what
 * fosvos_jf_counts gives for the masks (pred == k) and (gt == k) of frame n; labels above K belong to no object.  A pack
 * kernel writes the bit planes of every object ([N][K][H][ceil(W/64)] words twice: fosvos_jf_labels_workspace_bytes, 8-byte
 * aligned) and zeroes the counters, then the count kernel of fosvos_jf_counts runs on N K frames.  N K <= 65535,
 * 1 <= radius <= 63.  Two launches.
 *
 * fosvos_png_encode_indexed: labels uint8 [N,H,W] -> N standalone 8-bit palette PNG files (IHDR colour type 3): the file
 * of fosvos_png_encode with one PLTE chunk of the 256 RGB entries `palette` (uint8 [256,3], device memory) between IHDR and
 * the first IDAT, so it is 780 bytes longer: capacity >= fosvos_png_indexed_capacity_bytes.  huffman, lengths and workspace
 * (fosvos_png_workspace_bytes) as for fosvos_png_encode. */
#define FOSVOS_MAX_OBJECTS 16
int fosvos_merge_objects(const float *const *logits, int K, int N, int H, int W, uint8_t *labels, int device, void *stream);
size_t fosvos_jf_labels_workspace_bytes(int N, int K, int H, int W);
int fosvos_jf_counts_labels(const uint8_t *pred, const uint8_t *gt, int N, int K, int H, int W, int radius, int32_t *counts,
                            void *workspace, size_t workspace_bytes, int device, void *stream);
size_t fosvos_png_indexed_capacity_bytes(int N, int H, int W); /* per frame */
int fosvos_png_encode_indexed(const uint8_t *labels, const uint8_t *palette, int N, int H, int W, int huffman, uint8_t *out,
                              size_t capacity, int32_t *lengths, void *workspace, size_t workspace_bytes, int device,
                              void *stream);

/* ---- cleaning a mask by its shape: connected components and a temporal gate (ABI 33) -----------------------------------
 * The definitions are stated in numpy in util/mask_components.py; the tests compare with exact equality.  The mask of a
 * frame is logits >= 0 (a NaN is background, -0.0 foreground), its components are 8-connected, and a component's root is
 * the smallest raster index y * W + x of its pixels.
 *
 * fosvos_component_roots: logits fp32 [N,1,H,W] -> roots int32 [N,H,W]: -1 on the background, else the pixel's root.  The
 * labels are built in `roots` itself; workspace is not used (it may be null).  Three launches.
 *
 * fosvos_clean_components: a component is eligible when its area is >= min_area and - with the gate on - one of its pixels
 * lies inside the seed dilated by the disk of `radius` (0..63; 0 = touches the seed itself).  largest != 0 keeps of the
 * eligible components only the one of the largest area, on equal areas the one with the smaller root; otherwise all eligible
 * ones are kept.  out_logits fp32 [N,1,H,W]: a foreground pixel that is not kept becomes `fill` (finite and < 0), every
 * other value passes bit for bit; out_logits == logits is allowed.  kept uint8 [N,H,W] (may be null): 1 on kept pixels.
 *   chain == 0: seed uint8 [N,H,W] (non-zero = set) gates frame n with seed[n]; null: no gate.
 *   chain != 0: seed uint8 [1,H,W] or null gates frame 0; frame n > 0 is gated by the kept mask of frame n - 1.
 * The gate of a frame is off when its seed has no set pixel (decided on the device; the host never synchronises).
 * Launches: (1 with a seed) + per pass (1 with a gate) + 3 + (1 with largest) + 1; a chain makes one pass per frame,
 * otherwise all frames share one.  workspace: fosvos_components_workspace_bytes (0 for sizes outside the limits), 8-byte
 * aligned.  Limits: N <= 65535, H W < 2^31 (FOSVOS_E_SHAPE); radius, min_area >= 0, fill, null pointers (FOSVOS_E_ARG). */
size_t fosvos_components_workspace_bytes(int N, int H, int W);
int fosvos_component_roots(const float *logits, int N, int H, int W, int32_t *roots, void *workspace, size_t workspace_bytes,
                           int device, void *stream);
int fosvos_clean_components(const float *logits, const uint8_t *seed, int N, int H, int W, int radius, int min_area,
                            int largest, int chain, float fill, float *out_logits, uint8_t *kept, void *workspace,
                            size_t workspace_bytes, int device, void *stream);

/* ---- pseudo-labels for online adaptation: an exact Euclidean distance gate, and the labelling behind it -----------------
 * The definitions are stated in numpy in util/online_adapt.py (far_from, adapt_labels); the tests compare with exact
 * equality.  All distance arithmetic is int32.
 *
 * fosvos_distance_gate: mask uint8 [N,H,W] -> out uint8 [N,H,W].  A pixel q is "set" when (mask[q] != 0) != (invert != 0);
 * out[p] = 1 iff every set q of the frame has (py - qy)^2 + (px - qx)^2 > distance^2 (no set pixel: all 1).  With invert it
 * is the erosion of the mask by the Euclidean disk, the frame border not eating into it.  Two launches: a column pass
 * (vertical distances, uint16 saturated at distance + 1) and a row pass over a row staged in LDS.  The first N int32 words
 * of the workspace receive the frames' flags "the frame has a set pixel".
 *
 * fosvos_adapt_labels: logits fp32 [N,1,H,W], last_mask uint8 [N,H,W] -> label fp32 [N,1,H,W], void_px uint8 [N,1,H,W],
 * counts int32 [N,3] {positives, negatives, void} (zeroed by the call).  core = the mask eroded by the disk of `erode`
 * (erode == 0: last_mask != 0); a pixel further than neg_distance from every core pixel is a negative (label 0, void 0) -
 * unless the core is empty, which names no negatives; elsewhere logits >= pos_logit is a positive (label 1, void 0; a NaN
 * is not, +inf is); the rest is void (label 0, void 1).  Two launches, four with erode > 0; the last row pass labels and
 * counts (one atomic per workgroup and class).
 *
 * Limits: distance, neg_distance, erode 0..4095 (FOSVOS_E_ARG); 1 <= H, W <= 8192, 1 <= N <= 65535 (FOSVOS_E_SHAPE; the
 * workspace sizes are 0 outside them).  workspace: 16-byte aligned.  Nothing is launched when a check fails. */
size_t fosvos_distance_gate_workspace_bytes(int N, int H, int W);
int fosvos_distance_gate(const uint8_t *mask, int N, int H, int W, int distance, int invert, uint8_t *out, void *workspace,
                         size_t workspace_bytes, int device, void *stream);
size_t fosvos_adapt_labels_workspace_bytes(int N, int H, int W);
int fosvos_adapt_labels(const float *logits, const uint8_t *last_mask, int N, int H, int W, float pos_logit, int neg_distance,
                        int erode, float *label, uint8_t *void_px, int32_t *counts, void *workspace, size_t workspace_bytes,
                        int device, void *stream);

/* ---- the streamed output frames as JPEG files, encoded on the device --------------------------------------------------
 * fosvos_jpeg_encode: frames uint8 [N,H,W,3] BGR (what fosvos_overlay writes; components = 3) or [N,H,W] grey (components =
 * 1) -> N standalone baseline JFIF files: frame n's file is out[n * out_stride .. n * out_stride + lengths[n]), the bytes
 * behind it are left as they were.  The layout is stated in integers in util/jpeg_layout.py (the tests compare byte for
 * byte): libjpeg's 16-bit fixed-point colour rows, the Loeffler-Ligtenberg-Moschytz DCT with 13-bit constants, the Annex K
 * tables scaled by the IJG rule for `quality` (1..100), the standard Huffman tables.  sampling 444: an MCU is one block a
 * component, a restart interval 32 MCUs.  sampling 420 halves both chroma planes: an MCU is 16x16 pixels and six blocks
 * (Y Y Y Y Cb Cr), SOF0 says 2x2 1x1 1x1, the restart interval is 16 MCUs; chroma is libjpeg's h2v2 mean with the
 * alternating bias, luma blocks beyond ceil(W/8) x ceil(H/8) are dummies (DC of the block in front, no AC), and the file
 * is byte for byte libjpeg-turbo's for the same parameters.  A grey frame has no chroma: 420 gives the 444 file and sizes.
 * Any other sampling: the sizes are 0, the encode returns FOSVOS_E_ARG.  `frames` needs no alignment.
 *   out_stride bytes reserved per frame in `out`, >= fosvos_jpeg_capacity_bytes (the layout's size bound: header + 416 B a
 *              block - with 420 six blocks an MCU of the padded grid - + 2 B an interval; no image encodes to more; 0 for
 *              a shape the encoder does not take)
 *   lengths    int32 [N]
 *   workspace  fosvos_jpeg_workspace_bytes (4 B an interval), 4-byte aligned; what it and `out` held does not matter
 * H, W <= 65535 and a size bound below 2^31.  Integer arithmetic only; two launches on `stream`. */
size_t fosvos_jpeg_capacity_bytes(int N, int H, int W, int components, int sampling); /* per frame */
size_t fosvos_jpeg_workspace_bytes(int N, int H, int W, int components, int sampling);
int fosvos_jpeg_encode(const uint8_t *frames, int N, int H, int W, int components, int sampling, int quality, uint8_t *out,
                       size_t out_stride, int32_t *lengths, void *workspace, size_t workspace_bytes, int device, void *stream);

/* ---- JPEG files in, frames out: the decoder of the test pass's and the stream's input frames (ABI 28) ------------------
 * fosvos_jpeg_decode: N baseline JPEG files of ONE shape, component count and sampling -> frames uint8 [N,H,W,3] BGR
 * (components = 3) or [N,H,W] (components = 1) and status int32 [N].  util/jpeg_read.py states which files are taken
 * (probe), the bytes of the result and the status codes; the host parses the markers and sends
 *   bytes       the entropy-coded data of all files, n_bytes of it (< 2^31); stuffing and restart markers as in the files
 *   segments    int32 [n_segments][5]: file, byte offset into `bytes`, byte length, first MCU, MCU count - one row per
 *               restart interval (one per file without DRI), the rows of a file contiguous.  Rows are checked on the
 *               device: one that points outside `bytes` or the MCU grid decodes nothing and gives its file status 1
 *   tables      per file 2384 bytes: quant uint8 [3][64] (per component, natural order), dc_slot [3], ac_slot [3] (the
 *               slot, class * 4 + id, of each component's Huffman tables), 2 bytes unused, int32 first row and row count of
 *               the file in `segments`, then 8 slots of 272 bytes: the DHT payload (16 counts + symbols) as it stands in
 *               the file, zero-filled.  8-byte aligned
 *   sampling    444, or 420 (colour only: 2x2,1x1,1x1, W >= 5); a grey file ignores it
 *   status      per file 0, or the smallest non-zero status of its segments (1 bytes ran out, 2 no code matches, 3 a
 *               coefficient index beyond 63), or 5 (some coefficient x quant outside +-32767); the frame of a non-zero
 *               status is not meaningful
 *   workspace   fosvos_jpeg_decode_workspace_bytes (coefficients 128 B a block, the padded component planes, 4 B an MCU
 *               and 4 B per 32 blocks of status words), 16-byte aligned; 0 for a shape the decoder does not take
 * Argument checks come before any launch.  Integer arithmetic only; three launches on `stream`; every store is inside the
 * workspace, `frames` or `status`.
 * replaces: the PIL decode of src/dataloaders/davis_2016.py (make_img_gt_pair) and cv2.imread of src/run_webcam.py. */
size_t fosvos_jpeg_decode_workspace_bytes(int N, int H, int W, int components, int sampling);
int fosvos_jpeg_decode(const uint8_t *bytes, size_t n_bytes, const int32_t *segments, int n_segments, const void *tables, int N,
                       int H, int W, int components, int sampling, uint8_t *frames, int32_t *status, void *workspace,
                       size_t workspace_bytes, int device, void *stream);

/* ---- streaming inference: a raw camera frame in, the frame that is shown out -----------------------------------------
 * The per-frame arithmetic of src/run_webcam.py:81-133 (apply_network) on the device beside the nets; the definitions are
 * stated in numpy in util/frame_overlay.py.  One launch each on `stream`, no workspace, no library state.
 *
 * fosvos_frame_prep: frames uint8 [N,H,W,3] (BGR, as a camera or cv2.imread delivers them) -> image fp32 [N,3,H,W]:
 * image[n][c][y][x] = (float)frames[n][y][xs][c] - mean[c], xs = x, or W-1-x with `mirror`.  `mean` is read on the host
 * and travels in the kernel arguments.  Exactly numpy's float32(byte) - float32(mean).  3 B read, 12 B written per pixel.
 * replaces: cv2.flip, `img - mean_value` and to_tensor of src/run_webcam.py:71-72, 84-85, 101-107 and the fp32 upload.
 *
 * fosvos_overlay: frames as above and logits fp32 [N,1,H,W] (of the mirrored frame, if `mirror`) -> out uint8.
 *   mode 0  boolean overlay  out [N,H,W,3]: the (mirrored) frame with byte b of channel `channel` (0 b, 1 g, 2 r)
 *                            replaced by (uint8)min(b + (alpha * 255) * p, 255) in fp64, p = 1 where logit >= 0 (+0.0
 *                            and -0.0 alike) else 0
 *   mode 1  soft overlay     the same with p = 1 / (1 + exp(-(double)logit)), operation for operation in fp64
 *   mode 2  boolean mask     out [N,H,W]: 255 where logit >= 0 else 0 (`frames`, `mirror`, `channel`, `alpha` unused)
 *   mode 3  soft mask        out [N,H,W]: (uint8)(255 p + 0.5)
 * alpha finite and >= 0.  NaN-free logits only.  The boolean modes are exact; a soft byte can differ from the host's where
 * the fp64 value lies within an ulp of exp() of a rounding boundary.  7 B read and 3 B written per pixel (4 and 1 in the
 * mask modes).  Neither pointer needs more than its type's alignment: 16-byte accesses are used wherever they are aligned.
 * replaces: to_numpy, the >= 0.5 threshold and perform_overlay of src/run_webcam.py:89-98, 110-133 and the fp32 download. */
int fosvos_frame_prep(const uint8_t *frames, int N, int H, int W, int mirror, const float mean[3], float *image, int device,
                      void *stream);
int fosvos_overlay(const uint8_t *frames, const float *logits, int N, int H, int W, int mirror, int mode, int channel,
                   double alpha, uint8_t *out, int device, void *stream);

/* The same two with the net at a size of its own (opt-in): frames uint8 [N,Hf,Wf,3], the net's image and logits at [Hn,Wn],
 * 1 <= Hn <= Hf <= 8192 and 1 <= Wn <= Wf <= 8192 (FOSVOS_E_SHAPE otherwise).  util/frame_resample.py states both in numpy.
 *
 * fosvos_frame_prep_scaled: image fp32 [N,3,Hn,Wn] = the exact area average of the (mirrored) frame less the mean:
 *   S[i][j][c] = sum_y sum_x wy[i][y] wx[j][x] frames[n][y][x][c] in integers, w[j][s] = max(0, min((s+1) n_dst, (j+1) n_src)
 *   - max(s n_dst, j n_src)) along an axis of n_src source and n_dst output samples;
 *   image[n][c][i][j] = (float)((double)S / (double)(Hf Wf)) - mean[c].  Bit for bit the host's.
 *
 * fosvos_overlay_scaled: logits fp32 [N,1,Hn,Wn] -> out uint8 [N,Hf,Wf,3] (modes 0, 1) or [N,Hf,Wf] (modes 2, 3): fosvos_overlay
 * with the logit of an output pixel interpolated from the net's map, bilinear at half-pixel centres, clamped at the borders.
 *   Along an axis: num = (2x+1) n_src - n_dst, i0 = floor(num / (2 n_dst)), r = num mod (2 n_dst); num < 0: i0 = 0, r = 0;
 *   i0 >= n_src - 1: i0 = n_src - 1, r = 0; i1 = min(i0 + 1, n_src - 1); w0 = 2 n_dst - r, w1 = r.
 *   In fp64, in this order: top = a[y0][x0] wx0 + a[y0][x1] wx1, bot = a[y1][x0] wx0 + a[y1][x1] wx1, v = top wy0 + bot wy1.
 *   The boolean modes test v >= 0; the soft modes take the sigmoid of v / (double)(4 Hf Wf).
 * Alignment, alpha, channel, modes and error codes as above.  One launch each, no workspace, no library state. */
int fosvos_frame_prep_scaled(const uint8_t *frames, int N, int Hf, int Wf, int Hn, int Wn, int mirror, const float mean[3],
                             float *image, int device, void *stream);
int fosvos_overlay_scaled(const uint8_t *frames, const float *logits, int N, int Hf, int Wf, int Hn, int Wn, int mirror,
                          int mode, int channel, double alpha, uint8_t *out, int device, void *stream);

/* Following the object (opt-in): the net sees a WINDOW of every frame, and the window comes from device memory, so the host
 * never reads it.  util/frame_roi.py states all three in numpy.  `windows` is int32 [N][4] = (y0, x0, Hw, Ww) per frame, in
 * the coordinates of the picture the net sees (after `mirror`), 4-byte aligned.  A window is valid when Hn <= Hw <= Hf,
 * Wn <= Ww <= Wf, 0 <= y0 <= Hf - Hw and 0 <= x0 <= Wf - Ww; every kernel reads ANY other window - negative or overflowing
 * values included - as the whole frame (0, 0, Hf, Wf), so no loop bound or address depends on an unchecked value.  Sizes,
 * alignment, modes, alpha, channel and error codes as for the scaled entries.  No synchronisation, no host read.
 *
 * fosvos_frame_prep_window: fosvos_frame_prep_scaled of the window's pixels: weights of (Hw -> Hn) and (Ww -> Wn), one fp64
 *   division by Hw Ww.  Grid and LDS are those of fosvos_frame_prep_scaled at the same sizes.  The whole-frame window gives
 *   fosvos_frame_prep_scaled bit for bit, a window of the net's size float(byte) - mean of the crop.  One launch.
 *
 * fosvos_overlay_window: fosvos_overlay_scaled with the logits painted into the window: inside it the taps are those of
 *   (Hn -> Hw) and (Wn -> Ww) and the soft modes divide by 4 Hw Ww; outside it nothing is object (the frame's bytes, or a 0
 *   mask byte).  The grid is the frame's.  One launch.
 *
 * fosvos_window_next: logits fp32 [N,1,Hn,Wn] and the windows they were made through -> out int32 [N][4], the windows of the
 *   next frames (out == windows is allowed): the bounding box of logits >= 0 on the net's map (a NaN is not object, -0.0 is),
 *   mapped into the frame through the sanitised window, padded by min_pad + ceil(margin_permille max(box sides) / 1000),
 *   fitted into the smallest of the levels + 1 sizes Hn + (Hf - Hn) k / levels (widths likewise) that holds it, centred on
 *   the box and pushed into the frame; no object: the whole frame.  1 <= levels <= 64, 0 <= margin_permille <= 4000,
 *   0 <= min_pad <= 4095 (FOSVOS_E_ARG).  workspace: fosvos_window_next_workspace_bytes, 4-byte aligned; the entry
 *   initialises it.  An order-free min / max reduction by agent-scope atomics; nothing waits.  Two launches. */
int fosvos_frame_prep_window(const uint8_t *frames, const int32_t *windows, int N, int Hf, int Wf, int Hn, int Wn, int mirror,
                             const float mean[3], float *image, int device, void *stream);
int fosvos_overlay_window(const uint8_t *frames, const float *logits, const int32_t *windows, int N, int Hf, int Wf, int Hn,
                          int Wn, int mirror, int mode, int channel, double alpha, uint8_t *out, int device, void *stream);
size_t fosvos_window_next_workspace_bytes(int N);
int fosvos_window_next(const float *logits, const int32_t *windows, int N, int Hf, int Wf, int Hn, int Wn, int levels,
                       int margin_permille, int min_pad, int32_t *out, void *workspace, size_t workspace_bytes, int device,
                       void *stream);

/* Edge-aware upsampling of the stream's logits (opt-in): the guided filter with the frame as the guide.
 * util/guided_upsample.py states both entries in numpy; the coefficient maps and the boolean modes are compared with it bit
 * for bit.  Every fp64 operation is one IEEE operation of that file, in its order, uncontracted.  No synchronisation.
 *
 * fosvos_guided_coefficients (csrc/guided.hip): image fp32 [N,3,Hn,Wn] (what the prep made for the net) and logits fp32
 *   [N,1,Hn,Wn] -> coeff fp64 [N,2,Hn,Wn] = [abar, bbar]: the guide g = the sum of the three planes, the target p = the logit
 *   clipped to [-clip, clip] (a NaN is -clip), the linear model a g + b of every window of radius `radius` cut to the map,
 *   fitted with `eps`, then box-smoothed.  1 <= radius <= 8, 1e-3 <= eps <= 1e9, 0 < clip <= 1e4 (FOSVOS_E_ARG); sides of
 *   1..8192 (FOSVOS_E_SHAPE); image and logits 4-byte, coeff and workspace 8-byte aligned.  workspace:
 *   fosvos_guided_coefficients_workspace_bytes (the unsmoothed [a, b], fp64 [N,2,Hn,Wn]); every byte of it that is read was
 *   written by the call.  Two launches (fit, smooth) of 16 x 64 tiles with a halo of `radius` in 60 KB of LDS; no workgroup
 *   waits for another, no atomics.
 *
 * fosvos_overlay_guided (csrc/stream.hip): fosvos_overlay_scaled with, in place of the interpolated logit, v = A I + Bv: A and
 *   Bv are 4 Hf Wf times abar and bbar interpolated with the scaled overlay's taps, I = sum_c (byte_c - mean[c]) in fp64 of
 *   the (mirrored) frame pixel.  Modes, channel, alpha and sizes as for fosvos_overlay_scaled (Hn == Hf, Wn == Wf included),
 *   but the frames are read in EVERY mode (null: FOSVOS_E_ARG) and `mirror` applies to the mask modes too: the mask is that of
 *   the mirrored picture.  coeff 8-byte aligned.  One launch. */
size_t fosvos_guided_coefficients_workspace_bytes(int N, int Hn, int Wn);
int fosvos_guided_coefficients(const float *image, const float *logits, int N, int Hn, int Wn, int radius, double eps, double clip,
                               double *coeff, void *workspace, size_t workspace_bytes, int device, void *stream);
int fosvos_overlay_guided(const uint8_t *frames, const double *coeff, int N, int Hf, int Wf, int Hn, int Wn, int mirror, int mode,
                          int channel, double alpha, const float mean[3], uint8_t *out, int device, void *stream);

/* Several objects a stream (ABI 32, opt-in): the K logit maps of K per-object nets on the same frames (`logits` as for
 * fosvos_merge_objects: a host array of K device pointers that travel by value, 1 <= K <= FOSVOS_MAX_OBJECTS) are merged
 * and painted in one pass; no label map is written in between.  util/object_overlay.py states both in numpy; every byte is
 * exact.
 *   label    0 where no object's value is >= 0 (a NaN never is, -0.0 is), else 1 + the lowest k among those that hold the
 *            largest such value: the rule of fosvos_merge_objects
 *   pixel    label 0: the (mirrored) frame's three bytes.  Label k: per BGR channel c, with col = palette[k][2 - c] and the
 *            frame's byte b, in fp64 and one operation at a time: v = b + alpha * (col - b), out = (uint8)(v + 0.5)
 *   palette  uint8 [256][3] RGB in device memory; entries 1..K are read, once per workgroup
 *   alpha    finite, in [0, 1] (0: the frame; 1: the pure colour)
 *
 * fosvos_overlay_objects: logits[k] fp32 [N,1,H,W] -> out uint8 [N,H,W,3].  4 K + 3 B read and 3 B written per pixel.
 *
 * fosvos_overlay_objects_scaled: logits[k] fp32 [N,1,Hn,Wn]; the value of object k at an output pixel is the v of
 * fosvos_overlay_scaled (4 Hf Wf times the bilinear logit, fp64, that order), the taps taken once for all K maps.
 *   mode 0  out uint8 [N,Hf,Wf,3], the overlay
 *   mode 1  out uint8 [N,Hf,Wf], the label map (`frames`, `mirror`, `palette`, `alpha` unused)
 * Sizes as for fosvos_overlay_scaled.  The unscaled label map is fosvos_merge_objects.
 * Every map 4-byte aligned, nothing else needs more than its type's alignment.  One launch each, no workspace, no state. */
int fosvos_overlay_objects(const uint8_t *frames, const float *const *logits, int K, int N, int H, int W, int mirror,
                           const uint8_t *palette, double alpha, uint8_t *out, int device, void *stream);
int fosvos_overlay_objects_scaled(const uint8_t *frames, const float *const *logits, int K, int N, int Hf, int Wf, int Hn,
                                  int Wn, int mirror, int mode, const uint8_t *palette, double alpha, uint8_t *out, int device,
                                  void *stream);

/* Test-time ensemble of the test pass (opt-in; csrc/ensemble.hip): the net sees the frame mirrored and at other sizes, and its
 * answers are averaged back on the frame's grid.  util/test_ensemble.py states both entries in numpy; every output is
 * compared with it bit for bit.  Resampling is bilinear at half-pixel centres with the integer taps of
 * fosvos_overlay_scaled (util/frame_resample.taps, which also serve shrinking), every fp64 operation one IEEE operation of
 * that file, in its order, uncontracted.  `views` is a host array of V entries, 1 <= V <= FOSVOS_ENSEMBLE_MAX_VIEWS, that
 * travel by value in the kernel's arguments: data = device pointer fp32, h and w = the view's size, flip != 0 = mirrored
 * along W.
 *
 * fosvos_ensemble_views: image fp32 [N,3,H,W] -> V views fp32 [N,3,h_k,w_k].  A view of the frame's size is a (mirrored)
 *   copy, any other float32(v / (4 h_k w_k)) of the (mirrored) plane resampled in fp64.
 * fosvos_ensemble_merge: V logit maps fp32 [N,1,h_k,w_k] -> out fp32 [N,1,H,W] = float32((u_0 + u_1 + ... ) / V), summed in
 *   fp64 in the order of the views; u_k is the map itself where it has the frame's size and the map resampled to [H,W]
 *   otherwise, mirrored back where the view was flipped.  `out` must not overlap a map.
 *
 * One launch each, no workspace, no atomics, no state; a thread takes four consecutive output pixels of a row and stores
 * them as 16 bytes where they are aligned.  Every pointer 4-byte aligned.  Null pointer, V out of range: FOSVOS_E_ARG; a side
 * outside 1..8192, N outside 1..65535, more than 2^31 - 1 groups of four pixels in a launch: FOSVOS_E_SHAPE. */
#define FOSVOS_ENSEMBLE_MAX_VIEWS 8
typedef struct fosvos_ensemble_view {
    void *data;
    int h, w, flip;
} fosvos_ensemble_view;
int fosvos_ensemble_views(const float *image, int N, int H, int W, const fosvos_ensemble_view *views, int V, int device,
                          void *stream);
int fosvos_ensemble_merge(const fosvos_ensemble_view *views, int V, int N, int H, int W, float *out, int device, void *stream);

/* Refining the test pass's logits with a local CRF on the frame's colours (opt-in; csrc/crf.hip): mean-field inference over a
 * window of radius `radius` with an appearance kernel (near and alike in colour) and a smoothness kernel (near).
 * util/mask_crf.py states the arithmetic in numpy; `out` is compared with it bit for bit.  Every fp64 operation is one IEEE
 * operation of that file, in its order, uncontracted, and there is no transcendental: `tables` is the device copy of the fp64
 * vector mask_crf.tables made, [RGB 256 | A (2 radius + 1)^2 | B (2 radius + 1)^2 | D 2049] - the entry cannot see its length;
 * what it holds is only ever a value, never an index.
 *
 * fosvos_crf_refine: image fp32 [N,3,H,W] (the net's input: the frame minus `mean`, whose bytes the kernel takes back as the
 *   guide; a NaN is level 0) and logits fp32 [N,1,H,W] -> out fp32 [N,1,H,W] = float32(z^T); the unary is the logit clipped
 *   to [-clip, clip] (a NaN is -clip), z^t = (u + weight_appearance ma) + weight_smooth ms with ma and ms the two kernels'
 *   normalised messages of the beliefs of z^{t-1} (0.0 where a pixel's kernel mass is not positive).  `out` must not overlap
 *   an input.  1 <= iterations <= 10, 1 <= radius <= 5, weights in [0, 100], 0 < clip <= 1e4 (FOSVOS_E_ARG); sides of
 *   1..8192 (FOSVOS_E_SHAPE); image, logits and out 4-byte, tables and workspace 8-byte aligned.  workspace:
 *   fosvos_crf_refine_workspace_bytes (two fp64 maps [N,H,W], z^t by turns); every byte of it that is read was written by
 *   the call.  `iterations` launches of one kernel, 16 x 64 tiles with a halo of `radius` in 27 KB of LDS; the last writes
 *   `out`.  No workgroup waits for another, no atomics, no synchronisation. */
size_t fosvos_crf_refine_workspace_bytes(int N, int H, int W);
int fosvos_crf_refine(const float *image, const float *logits, const double *tables, int N, int H, int W, int iterations,
                      int radius, double weight_appearance, double weight_smooth, double clip, const float mean[3], float *out,
                      void *workspace, size_t workspace_bytes, int device, void *stream);

/* A joint CRF over the objects of a frame (opt-in; csrc/crf.hip): ONE mean-field CRF over the labels 0..K (0 = background) in
 * the place of K fosvos_crf_refine calls and fosvos_merge_objects.  util/label_crf.py states the arithmetic in numpy; labels
 * and scores are compared with it bit for bit, under the rules of fosvos_crf_refine.  `tables` is the device copy of the fp64
 * vector label_crf.tables made, [RGB 256 | A (2 radius + 1)^2 | B (2 radius + 1)^2 | E 2049]; every index into it is clamped.
 *
 * fosvos_crf_labels: image fp32 [N,3,H,W] as for fosvos_crf_refine; logits[k] fp32 [N,1,H,W] of net k (`logits` as for
 *   fosvos_merge_objects: a host array of K device pointers that travel by value, 1 <= K <= FOSVOS_MAX_OBJECTS) -> labels uint8
 *   [N,H,W] and, where `scores` is not NULL, scores fp32 [N,K+1,H,W] = float32(z^T).  U_0 = 0, U_k the logit of net k - 1
 *   clipped to [-clip, clip] (a NaN is -clip); the beliefs of a pixel are a soft-max of its z, piecewise linear on E;
 *   z^t_l = (U_l + weight_appearance ma_l) + weight_smooth ms_l.  The label: the largest z^T, an object before the background
 *   and the lowest object among equal ones (the rule of fosvos_merge_objects).  Ranges, codes and alignments as for
 *   fosvos_crf_refine (the scores 4-byte aligned); K outside its range is FOSVOS_E_ARG.  workspace:
 *   fosvos_crf_labels_workspace_bytes = 16 (K + 1) N H W (two sets of K + 1 fp64 maps [N,K+1,H,W], z^t by turns); every byte
 *   of it that is read was written by the call.  `iterations` launches of one kernel, 16 x 64 tiles with a halo of `radius`;
 *   a workgroup walks the labels in chunks of four (71.5 KB of LDS) and computes a neighbour's appearance weight once per
 *   chunk; the last launch writes the labels and the scores.  No workgroup waits for another, no atomics, no synchronisation. */
size_t fosvos_crf_labels_workspace_bytes(int N, int K, int H, int W);
int fosvos_crf_labels(const float *image, const float *const *logits, int K, const double *tables, int N, int H, int W,
                      int iterations, int radius, double weight_appearance, double weight_smooth, double clip, const float mean[3],
                      uint8_t *labels, float *scores, void *workspace, size_t workspace_bytes, int device, void *stream);

/* Measuring how the picture moved between two frames and moving a mask along with it (opt-in; csrc/motion.hip): full-search
 * block matching on the frames' luma and a per-block warp, all in integers.  util/block_motion.py states the arithmetic in
 * numpy; every output is compared with it bit for bit.  Each entry is ONE launch on `stream`; no workspace, no atomics, no
 * workgroup waits for another, no synchronisation.  Sides of 1..8192 (FOSVOS_E_SHAPE).
 *
 * fosvos_motion_luma: image fp32 [N,3,H,W] (the net's input: the frame minus `mean`, whose bytes are taken back as
 *   fosvos_crf_refine takes them; a NaN is level 0) -> out u8 [N,H,W], Y = (29 g0 + 150 g1 + 77 g2 + 128) >> 8.  The image
 *   4-byte aligned.
 * fosvos_motion_estimate: prev, cur u8 [N,H,W] -> field i8 [N,Hb,Wb,2] = (dy, dx) and cost i32 [N,Hb,Wb] (4-byte aligned),
 *   Hb = ceil(H / block), Wb = ceil(W / block); pair n is (prev[n], cur[n]), so consecutive frames of one buffer are two
 *   pointers one plane apart.  Block (by, bx) owns the pixels P of its square that lie in the frame; a candidate d in
 *   [-search, search]^2 counts iff P + d lies wholly in the frame (skipped otherwise, never clamped); SAD(d) = sum over P of
 *   |cur[p] - prev[p + d]|, score(d) = SAD(d) + (d != 0 ? (zero_bias |P|) >> 4 : 0); the winner is the smallest
 *   (score, dy^2 + dx^2, dy, dx); cost is its SAD.  cur[p] ~ prev[p + field].  block 8 or 16, 1 <= search <= 16,
 *   0 <= zero_bias <= 255 (FOSVOS_E_ARG).  16 x 64 tiles with a halo of `search` in 5.7 KB of LDS; a wave owns a block, its
 *   lanes share out the candidates.
 * fosvos_motion_warp: mask u8 [N,H,W] (non-zero = set) and field i8 [N,Hb,Wb,2] (ANY values) -> out u8 [N,H,W] of 0 and 1:
 *   out[y, x] = mask[y + dy, x + dx] != 0 with the pixel's block's (dy, dx), 0 where the source lies outside the frame (tested
 *   before the read).  block 8 or 16; `out` must not overlap `mask` (FOSVOS_E_ARG). */
int fosvos_motion_luma(const float *image, const float mean[3], int N, int H, int W, uint8_t *out, int device, void *stream);
int fosvos_motion_estimate(const uint8_t *prev, const uint8_t *cur, int N, int H, int W, int block, int search, int zero_bias,
                           int8_t *field, int32_t *cost, int device, void *stream);
int fosvos_motion_warp(const uint8_t *mask, const int8_t *field, int N, int H, int W, int block, uint8_t *out, int device,
                       void *stream);

/* ---- thin-channel ResNet inference path (OSVOS_RESNET and the nets prune.py derives from it) ------
 * Activations: bf16 NHWC [N,H,W,Cp] with Cp = channels rounded up to a multiple of 8, padded channels zero.
 * Eval-mode BatchNorm is folded into the conv in front of it when the weights are packed:
 *   s[o] = bn_weight[o] / sqrt(bn_var[o] + eps);  w'[o] = w[o] * s[o];  b'[o] = bn_bias[o] - bn_mean[o] * s[o]
 *   (+ conv_bias[o] * s[o]; bn_* all NULL: no BatchNorm, b' = conv_bias or 0).
 * Packed image: uint32 [Cip/8][k*k][4][Cop] (two bf16 input channels per word), fosvos_conv2d_packed_dwords words;
 * folded bias: fosvos_conv2d_bias_elems floats (zero beyond Co).  The contraction runs on the vector ALU
 * (v_dot2c_f32_bf16, fp32 accumulate) with any channel counts - these layers are too thin for the MFMA path.
 * replaces: nn.Conv2d + nn.BatchNorm2d (+ residual add) + nn.ReLU of torchvision's BasicBlock / Bottleneck as wired by
 *           src/networks/osvos_resnet.py:91-121,187-216, and the side_prep convs of :135. */
/* The fold alone (fp32 OIHW in, fp32 OIHW out, bias_out[Co]): for 3x3 stride-1 layers whose channel counts fit the MFMA
 * path (Ci % 32 == 0, Co % 64 == 0), which then go through fosvos_pack_conv3x3_weights and fosvos_conv3x3_fwd[_add]. */
int fosvos_fold_conv_bn(const float *w_oihw, int Co, int Ci, int k, const float *conv_bias, const float *bn_weight,
                        const float *bn_bias, const float *bn_mean, const float *bn_var, float eps, float *w_folded,
                        float *bias_out, int device, void *stream);
size_t fosvos_conv2d_packed_dwords(int out_ch, int in_ch, int k);
size_t fosvos_conv2d_bias_elems(int out_ch);
int fosvos_pack_conv2d_bn(const float *w_oihw, int Co, int Ci, int k /* 1 or 3 */, const float *conv_bias,
                          const float *bn_weight, const float *bn_bias, const float *bn_mean, const float *bn_var,
                          float eps, uint32_t *w_packed, float *bias_out, int device, void *stream);
/* y[N,Ho,Wo,Cop] = act(conv_k,stride,pad=k/2(x) + bias + addend); Ho = (H + 2 (k/2) - k) / stride + 1.
 * addend: bf16 [N,Ho,Wo,Cop] or NULL (the residual branch).  flags: FOSVOS_CONV_RELU, FOSVOS_CONV_OUT_F32 (3x3
 * stride 1 without addend only: the fp32 side maps the head reads). */
int fosvos_conv2d_fwd(const uint16_t *x, const uint32_t *w_packed, const float *bias, const uint16_t *addend, void *y,
                      int N, int H, int W, int Ci, int Co, int k, int stride, unsigned flags, int device, void *stream);
/* What fosvos_conv2d_fwd launches for a shape (host arithmetic only; test plumbing like fosvos_conv3x3_plan): output
 * channels per thread (cob: 64, 32, 16 or 8), threads per K slice (64 or 256), K slices of a workgroup (1, 2, 4 or 8: the
 * input-channel chunks of 8 are dealt round-robin to the slices) and workgroups.  The plan does not depend on the
 * flags.  k = 7, stride = 2, Ci = 3 asks for fosvos_conv7x7s2_first_fwd instead: cob / threads / slices / workgroups are
 * those of its FOSVOS_CONV_FP32_MATH form (which is also what more than 64 channels take), mfma_frag_blocks (16-channel
 * fragment blocks, 1..4) and mfma_workgroups those of the default MFMA form (both 0 where it does not apply). */
typedef struct fosvos_conv2d_plan_info {
    int cob, threads, slices, workgroups;
    int mfma_frag_blocks, mfma_workgroups;
} fosvos_conv2d_plan_info;
int fosvos_conv2d_plan(int N, int H, int W, int Ci, int Co, int k, int stride, fosvos_conv2d_plan_info *out);
/* First layer: 7x7 stride 2 pad 3 on the fp32 NCHW frame (3 channels) + folded BatchNorm (+ ReLU) -> bf16 NHWC
 * [N,(H-1)/2+1,(W-1)/2+1,Cop].  Packed image (fosvos_conv7x7_packed_elems floats): fp32 [49*3][Cop], then the same
 * filter as bf16 MFMA fragments.  By default (Cop <= 64) the layer runs on the matrix cores with the frame rounded to
 * bf16 like every other activation of the path; FOSVOS_CONV_FP32_MATH keeps frame and weights fp32 on the vector ALU.
 * replaces: layer_base conv1 + bn1 + relu (src/networks/osvos_resnet.py:92-94). */
size_t fosvos_conv7x7_packed_elems(int out_ch);
int fosvos_pack_conv7x7_bn(const float *w_oihw, int Co, const float *bn_weight, const float *bn_bias,
                           const float *bn_mean, const float *bn_var, float eps, float *w_packed, float *bias_out,
                           int device, void *stream);
int fosvos_conv7x7s2_first_fwd(const float *frame, const float *w_packed, const float *bias, uint16_t *y, int N, int H,
                               int W, int Co, unsigned flags, int device, void *stream);
/* layer_base in ONE launch: conv 7x7/2 + folded BatchNorm + ReLU + MaxPool2d(3, 2, 1) -> bf16 NHWC
 * [N,Hp,Wp,Cop], Hp = ((H-1)/2+1 - 1)/2 + 1; the conv map is never written.  MFMA form only (Cop <= 64); same bits as
 * fosvos_conv7x7s2_first_fwd followed by fosvos_maxpool3x3s2_fwd.
 * replaces: layer_base (src/networks/osvos_resnet.py:91-96). */
int fosvos_conv7x7s2_pool_first_fwd(const float *frame, const float *w_packed, const float *bias, uint16_t *y_pooled, int N,
                                    int H, int W, int Co, int device, void *stream);
/* MaxPool2d(kernel 3, stride 2, padding 1) on bf16 NHWC, C % 8 == 0: [N,H,W,C] -> [N,(H-1)/2+1,(W-1)/2+1,C].
 * replaces: layer_base maxpool (src/networks/osvos_resnet.py:95). */
int fosvos_maxpool3x3s2_fwd(const uint16_t *x, uint16_t *y, int N, int H, int W, int C, int device, void *stream);
/* Side-output head with a free stride per scale (OSVOS_RESNET: 4, 8, 16, 32), forward only:
 *   fused[n,0,Y,X]  = fuse_b + sum_s sum_c sum_taps filt[s][ky][kx][c] * side[s][n,i,j,c]
 *   side_out[s][..] = sum_taps filt1[s][ky][kx] * (dsn_b[s] + sum_c dsn_w[s][c] * side[s][n,i,j,c])   (optional)
 * over the taps of a transposed conv with kernel 2 f_s and stride f_s, centre-cropped to H x W as the reference
 * does.  filt[s] = [2f][2f][16] is the upscale_side_prep[s] weight CONTRACTED with the fuse weights of scale s
 * (G[ky][kx][ci] = sum_co fuse_w[16 s + co] * W[ci][co][ky][kx]; both maps are linear), so the full 16 -> 16
 * transposed conv, the concat and the 1x1 fuse cost one filter.  filt1[s] = [2f][2f].
 * replaces: upscale_side_prep, score_dsn, upscale_score_dsn, center_crop, torch.cat, layer_fuse
 *           (src/networks/osvos_resnet.py:53-66). */
int fosvos_deconv_head_fwd(const float *const side[4], const int hs[4], const int ws[4], const int stride[4],
                           const float *const filt[4], const float *const filt1[4], const float *dsn_w /*[4][16]*/,
                           const float *dsn_b /*[4]*/, const float *fuse_b /*[1]*/, float *fused,
                           float *const side_out[4] /* all NULL or all set */, int N, int H, int W, int device,
                           void *stream);

/* Whole-network forward of the ResNet family: ONE call issues every kernel of OSVOS_RESNET.forward (first conv, pool,
 * every block with its residual branch, the four side_prep convs, the head) over a caller-provided arena.  The
 * structs live in HOST memory for the duration of the call and hold device pointers to images made by the pack
 * calls above; `blocks` is a host array listing the blocks stage after stage.
 * replaces: OSVOS_RESNET.forward (src/networks/osvos_resnet.py:42-68) as driven from Python. */
typedef struct fosvos_conv2d_desc {
    const void *w_packed;       /* kind 0: fosvos_pack_conv2d_bn image; kind 1: fosvos_pack_conv3x3_weights forward image */
    const float *bias;          /* kind 0: fosvos_conv2d_bias_elems floats; kind 1: Co floats */
    int Ci, Co, k, stride;
    int kind;                   /* 0 = vector-ALU direct conv, 1 = MFMA implicit GEMM (3x3, Ci % 32 == 0, Co % 64 == 0 or Co = 32; Co = 16
                                 * for side_prep; stride 2 through fosvos_conv3x3_s2_fwd) */
} fosvos_conv2d_desc;
typedef struct fosvos_resnet_block {
    fosvos_conv2d_desc conv[3]; /* conv+bn(+relu) chain; the last one adds the residual before its ReLU */
    int n_convs;                /* 2 = BasicBlock, 3 = Bottleneck */
    int has_down;
    fosvos_conv2d_desc down;    /* 1x1 downsample conv + bn of the residual branch */
} fosvos_resnet_block;
typedef struct fosvos_resnet_net {
    const float *first_w;       /* fosvos_pack_conv7x7_bn image */
    const float *first_b;
    int first_co;
    int first_fp32_math;        /* != 0: FOSVOS_CONV_FP32_MATH for the first layer */
    int first_unfused;          /* 0: first layer and max pool in one launch (fosvos_conv7x7s2_pool_first_fwd: the MFMA form
                                 * only, so first_fp32_math must be 0, and at most 64 channels; it pays up to 32); != 0: two */
    int blocks_per_stage[4];
    const fosvos_resnet_block *blocks;
    fosvos_conv2d_desc side[4]; /* side_prep: 3x3 stride 1, Co = 16 */
    const float *filt[4];       /* as fosvos_deconv_head_fwd */
    const float *filt1[4];
    int stride[4];
    const float *dsn_w, *dsn_b, *fuse_b;
} fosvos_resnet_net;
size_t fosvos_resnet_arena_bytes(const fosvos_resnet_net *net, int N, int H, int W);
/* fused: [N,1,H,W] fp32; side_out: four [N,1,H,W] fp32 buffers or NULL.
 * aux_stream (a second hipStream_t of the same device, or NULL): when given, the kernels the trunk does not wait for
 * right away - each stage's side_prep conv and the 1x1 downsample convs - are issued on it beside the trunk's chain
 * (thin layers leave most of the chip idle), ordered by events of `ctx` (required with an aux_stream, else it may be
 * NULL); the caller sees ordinary single-stream semantics on `stream`.  Measured on MI355X at 1920x1080 this
 * costs 0.1 ms per frame more than it saves (cross-stream waits), so the shipped host passes NULL. */
int fosvos_resnet_forward(const fosvos_resnet_net *net, const float *frame, int N, int H, int W, void *arena,
                          size_t arena_bytes, float *fused, float *const side_out[4], int device, void *stream,
                          fosvos_ctx *ctx, void *aux_stream);

/* ---- whole-network entry points ------------------------------------------------------------------
 * The reference drives ~60 torch.nn calls per forward from Python (src/networks/osvos_vgg.py:61-83) and
 * autograd replays them backward.  Here the layer loop itself is native: ONE call issues every kernel of
 * OSVOS_VGG.forward, ONE call every kernel of its backward, over a caller-provided arena (activations,
 * activation gradients, op workspaces; layout private to the library, size from fosvos_vgg_arena_bytes).
 * The structs hold device pointers only and live in HOST memory for the duration of the call.
 * Conv index c = 0..12 runs conv1_1 .. conv5_3; side index i = 0..3 hangs off stages 2..5.
 * replaces: OSVOS_VGG.forward and its autograd graph. */
typedef struct fosvos_vgg_weights {
    const float *conv_w[13];      /* fp32 OIHW masters (only conv_w[0] is read by a kernel; the rest via images) */
    const float *conv_b[13];      /* fp32 [Co] */
    const uint16_t *conv_wf[13];  /* packed forward images ([0] unused) */
    const uint16_t *conv_wd[13];  /* packed dgrad images  ([0] unused) */
    const float *side_b[4];
    const uint16_t *side_wf[4];
    const uint16_t *side_wd[4];
    const float *filt[4];         /* [k][k][16] per-channel deconv filters */
    const float *filt1[4];        /* [k][k] */
    const float *dsn_w;           /* [4][16] */
    const float *dsn_b;           /* [4] */
    const float *fuse_w;          /* [64] */
    const float *fuse_b;          /* [1] */
    int filt_uniform;             /* bit s: filt[s]'s 16 channel filters are identical (see fosvos_head_fwd) */
} fosvos_vgg_weights;

typedef struct fosvos_vgg_grads {
    float *conv_w[13];            /* fp32 OIHW */
    float *conv_b[13];
    float *side_w[4];             /* [16,C,3,3] */
    float *side_b[4];
    float *dsn_w;                 /* [4][16] or NULL when no side-output gradient flows */
    float *dsn_b;                 /* [4] or NULL */
    float *fuse_w;                /* [64] */
    float *fuse_b;                /* [1] */
    int accumulate;               /* != 0: add into the buffers (gradient accumulation), else overwrite */
    int defer_join;               /* != 0 with an aux_stream: do NOT make `stream` wait for the weight gradients at the
                                   * end of the call; the caller joins (stream waits on aux_stream) before it reads
                                   * them, and must not reuse this arena before that.  Lets the next forward pass
                                   * (other arena, same weights) overlap the tail of the weight-gradient kernels. */
    int bucket_events;            /* != 0: publish the gradients in four pieces as the pass finishes them (stage 5,
                                   * stage 4, stage 3, the rest) so that a data-parallel caller can start each piece's
                                   * all-reduce early: see fosvos_vgg_grad_bucket_wait. */
    int last_pass_of_cycle;       /* != 0: a hint - no forward pass follows this backward pass before the optimizer step
                                   * (the last one of an accumulation cycle), so the weight-gradient kernels of the first
                                   * two stages, which run after the data-gradient chain has ended, may take the whole
                                   * chip (256 pixel splits instead of the shared-chip count).  Results differ only in
                                   * the order of the fp32 sums over splits. */
} fosvos_vgg_grads;

size_t fosvos_vgg_arena_bytes(int N, int H, int W);
/* fused: [N,1,H,W] fp32; side_out: four [N,1,H,W] fp32 buffers or NULL.  The arena keeps what backward needs.
 * A batch (N >= 2) runs as two chains of ceil(N/2) and floor(N/2) frames - each layer is launched once per chain - so
 * that a frame's arithmetic (tile plan, K split) is the same whether or not a second stream is there to run the chains
 * side by side (fosvos_vgg_forward_streams). */
int fosvos_vgg_forward(const fosvos_vgg_weights *w, const float *frame, int N, int H, int W, void *arena,
                       size_t arena_bytes, float *fused, float *const side_out[4], int device, void *stream);
/* The same pass with a second stream of the same device (or NULL = fosvos_vgg_forward): the second chain of frames runs on
 * aux_stream beside the first (one frame: only its four side_prep convs, beside the next stage's backbone convs); `stream`
 * waits for it (events of `ctx`, whose device the call runs on) in front of the head, so the caller sees single-stream
 * semantics on `stream`.  Results are bit-identical to fosvos_vgg_forward. */
int fosvos_vgg_forward_streams(fosvos_ctx *ctx, const fosvos_vgg_weights *w, const float *frame, int N, int H, int W,
                               void *arena, size_t arena_bytes, float *fused, float *const side_out[4], void *stream,
                               void *aux_stream);
/* d_fused / d_side_out: upstream gradients ([N,1,H,W] fp32; d_fused or all four d_side_out may be NULL).
 * Must follow a fosvos_vgg_forward on the same arena, frame and shape; runs on ctx's device.
 * aux_stream (a second hipStream_t of the same device, or NULL): when given, every weight-gradient kernel is
 * issued on it while the data-gradient chain stays on `stream`; the two are ordered by events (a layer's wgrad
 * waits for that layer's output gradient; `stream` waits for the last wgrad before the call's work is complete
 * in stream order), so the caller sees ordinary single-stream semantics on `stream`.  The events are the context's:
 * the library itself keeps no state between calls. */
int fosvos_vgg_backward(fosvos_ctx *ctx, const fosvos_vgg_weights *w, const fosvos_vgg_grads *g, const float *frame, int N,
                        int H, int W, void *arena, size_t arena_bytes, const float *d_fused,
                        const float *const d_side_out[4], void *stream, void *aux_stream);
/* Pass flags of the _flags entries below (the entries above are the same calls with flags = 0). */
#define FOSVOS_VGG_COMPACT_STAGE1 1u /* conv1_2 writes no dense output: see fosvos_vgg_stage1_compact */
/* 1 if a pass of this shape with these flags runs stage 1 in its COMPACT form: conv1_2's forward writes the pooled map and
 * the pool's winner codes (fosvos_conv3x3_fwd_pool_codes; the codes lie at the start of the arena's act[1] region, whose rest
 * is then left untouched) and the backward pass routes the pooled gradient with fosvos_maxpool2x2_ceil_bwd_codes.  Only
 * where FOSVOS_VGG_COMPACT_STAGE1 is set and the conv1_2 launch of EVERY forward chain (ceil(N/2) and floor(N/2) frames for
 * N >= 2, else N) is one the persistent kernel takes; otherwise 0 and the whole pass is dense, exactly as with flags = 0.
 * Forward and backward both decide by this function: give them the same flags.  The arena layout does not depend on it. */
int fosvos_vgg_stage1_compact(unsigned flags, int N, int H, int W);
int fosvos_vgg_forward_flags(const fosvos_vgg_weights *w, const float *frame, int N, int H, int W, void *arena,
                             size_t arena_bytes, float *fused, float *const side_out[4], int device, void *stream,
                             unsigned flags);
int fosvos_vgg_forward_streams_flags(fosvos_ctx *ctx, const fosvos_vgg_weights *w, const float *frame, int N, int H, int W,
                                     void *arena, size_t arena_bytes, float *fused, float *const side_out[4], void *stream,
                                     void *aux_stream, unsigned flags);
int fosvos_vgg_backward_flags(fosvos_ctx *ctx, const fosvos_vgg_weights *w, const fosvos_vgg_grads *g, const float *frame,
                              int N, int H, int W, void *arena, size_t arena_bytes, const float *d_fused,
                              const float *const d_side_out[4], void *stream, void *aux_stream, unsigned flags);
/* Make `stream` wait until gradient bucket `bucket` of the LAST fosvos_vgg_backward ON THIS CONTEXT (called with
 * grads.bucket_events != 0) is complete in its buffers: 0 = conv5_1..conv5_3 (stages.4), 1 = conv4_1..conv4_3
 * (stages.3), 2 = conv3_1..conv3_3 (stages.2) - 97 % of the gradient bytes, each published as the pass finishes it - then
 * 3 = conv1_1..conv2_2, 4 = side_prep / score_dsn / fuse (3 and 4 complete together, at the end of the pass, on both of
 * its streams).  Nothing blocks on the host.  The reference has no collective; this is the hook the
 * RCCL gradient all-reduce of BASELINE.json's north_star overlaps the backward pass with. */
int fosvos_vgg_grad_bucket_wait(fosvos_ctx *ctx, int bucket, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FOSVOS_HIP_H */
