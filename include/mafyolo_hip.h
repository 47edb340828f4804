/*
 * mafyolo_hip.h — C-ABI of libmafyolo_hip.so: the MI355X (gfx950) native hot path of MAF-YOLO.
 *
 * The reference (yang-0201/MAF-YOLO) is pure PyTorch: it has no FFI layer, its "operator API" for
 * this path is the Python surface Model.forward() / non_max_suppression().  This header is the
 * boundary a maintainer would bind (ctypes stub in INTEGRATION.md) to run that path natively:
 * plain pointers and sizes, no torch types.  All pointers are DEVICE pointers unless noted; all
 * launches go to the hipStream_t passed in (pass the framework's current stream); nothing here
 * allocates device memory, synchronises the device or keeps references after return, except
 * maf_engine_* which keeps a host-side copy of the op list.
 *
 * Every entry point returns 0 on success or a negative MAF_E_* code; maf_last_error() returns a
 * thread-local message.  Reference lines cited are relative to /root/reference.
 *
 * Activation layout is NHWC ("pixels x channels"), element type f16 or f32 (MAF_F16 / MAF_F32),
 * fp32 accumulation everywhere.  A tensor view is (ptr, stride, coff): channel c of pixel m lives
 * at ptr[m*stride + coff + c] — producers write straight into channel slices of wider buffers, so
 * torch.cat / Tensor.split / nn.Upsample / MaxPool2d(2) of the reference (common.py:154,670,940,944;
 * MAF-YOLO-n.yaml:21,26) never materialise.
 */
#ifndef MAFYOLO_HIP_H
#define MAFYOLO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* maf_stream_t;              /* hipStream_t */

enum { MAF_F16 = 0, MAF_F32 = 1, MAF_U8 = 2 };
enum { MAF_ACT_NONE = 0, MAF_ACT_RELU = 1, MAF_ACT_SILU = 2, MAF_ACT_SIGMOID = 3 };
enum { MAF_SRC_DIRECT = 0,               /* source has the op's H x W grid                              */
       MAF_SRC_UP2 = 1,                  /* source is H/2 x W/2, read through nearest x2 upsample       */
       MAF_SRC_POOL2 = 2,                /* source is 2H x 2W, read through MaxPool2d(2,2)              */
       MAF_SRC_SUB2 = 3,                 /* source is 2H x 2W, pixel (2y, 2x) is read: a 1x1 conv with stride 2 (RepVGGBlock.rbr_1x1)   */
       MAF_SRC_PAIRS = 4 };              /* source has the op's grid, stored as PIXEL PAIRS: [B][H][W/2][stride][2] halfs, channel c of pixel x at
                                            ((b H + y) W + (x & ~1)) stride + 2 (coff + c) + (x & 1) — what a CONV1X1 with out_pairs = 1 writes and a
                                            DWCONV with tile_p = -4 reads (csrc/dwconv_p2.hip); fp16, even W, the buffer holds nothing else              */
enum { MAF_OP_STEM = 0,                  /* RepVGGBlock L0 deploy form: 3x3 s2 conv on the NCHW image   */
       MAF_OP_CONV1X1 = 1,               /* Conv 1x1 (+bias+act) over up to 4 concatenated sources      */
       MAF_OP_CONV3X3S2 = 2,             /* RepVGGBlock / ConvWrapper 3x3 stride 2 pad 1 (+bias+act)    */
       MAF_OP_DWCONV = 3,                /* merged DilatedReparamBlock: depth-wise k x k s1 (+bias+act) */
       MAF_OP_SPPF_POOL = 4,             /* three chained MaxPool2d(5,1,2) into concat slices           */
       MAF_OP_DECODE = 5,                /* Detect_yaml eval branch: DFL decode -> [B,A,5+nc] fp32      */
       MAF_OP_BOTTLENECK = 6,            /* fused DepthBottleneckUni: 1x1 -> depth-wise k x k -> 1x1    */
       MAF_OP_CONV1DW = 7,               /* first half of a DepthBottleneckUni: 1x1 (c -> 3c) + SiLU -> depth-wise k x k + SiLU */
       MAF_OP_HEADTAIL = 8,              /* one detection level: {cls,reg}_conv_s -> {cls,reg}_pred -> sigmoid / DFL decode into the prediction rows */
       MAF_OP_STEM2 = 9,                 /* backbone.0 + backbone.1: image -> 1/4-resolution map, the 1/2-resolution tensor stays in LDS */
       MAF_OP_CONV3X3S2_DGRAD = 10 };    /* training: data gradient of a 3x3 stride-2 pad-1 conv (gather form, no atomics)              */
/* maf_op_t.tile_k of MAF_OP_CONV1X1 / MAF_OP_CONV3X3S2: the kernel variant (described with the kinds below; 0 = MAF_CONV_GENERIC in the forward dispatch) */
enum { MAF_CONV_GENERIC = 1,             /* each wave reduces all of K                                   */
       MAF_CONV_LDS = 2,                 /* the workgroup shares each k-step's weight fragments through LDS */
       MAF_CONV_STREAM = 3,              /* persistent waves, cross-tile prefetch (1x1, one direct source) */
       MAF_CONV_SPLITK = 4,              /* the 4 waves of a workgroup split K (tile_p = 1)              */
       MAF_CONV_STREAM_LDS = 5,          /* persistent waves, the channel tile's weights resident in LDS (1x1) */
       MAF_CONV3_LDS = 6,                /* 3x3 s2: all weights and the input patch in LDS               */
       MAF_CONV3_WREG = 7,               /* 3x3 s2: all weights in registers, patches by DMA             */
       MAF_CONV_DMA = 8 };               /* MAF_CONV_LDS with the fragments arriving by DMA              */
/* maf_op_t.tile_p < 0 of MAF_OP_DWCONV: the kernel (-3 left the library); their tile_k = tile rows * 256 + channels per block (DOT2) or waves per
 * workgroup (PAIRS), the latter + MAF_DW_P2_STAGED for staged stores */
enum { MAF_DW_MFMA = -1, MAF_DW_DOT2 = -2, MAF_DW_PAIRS = -4 };
enum { MAF_DW_P2_STAGED = 128 };
#define MAF_DW_TILE_ROWS(tile_k) ((tile_k) >> 8)
enum { MAF_E_ARG = -1, MAF_E_UNSUPPORTED = -2, MAF_E_HIP = -3 };

typedef struct {
    const void* ptr;
    int32_t C;        /* channels consumed from this source                         */
    int32_t stride;   /* elements per pixel of the underlying buffer                */
    int32_t coff;     /* first channel                                              */
    int32_t mode;     /* MAF_SRC_*                                                  */
} maf_src_t;

/*
 * One launch of the plan.  Fields not used by a kind are ignored.
 *
 * MAF_OP_STEM       replaces backbone.0.rbr_reparam + ReLU (yolov6/layers/common.py:216-217).
 *                   src[0].ptr = image [B,3,2H,2W] NCHW of type in_dtype (f16/f32, or u8 scaled by
 *                   1/255 = evaler.py:161-163 folded in); w = fp32 [27][Cout] (k = (c*3+ky)*3+kx).
 * MAF_OP_CONV1X1    replaces Conv.forward_fuse (common.py:49-50) and the plain nn.Conv2d preds
 *                   (common.py:1331,1335).  w = MFMA-fragment-packed (maf_pack_* in pack.py),
 *                   K = concat of the sources' channels in order (= torch.cat order).
 *                   tile_k = 5 (fp16, 2 <= K / 32 <= 24, K / 32 * tile_c <= 160): persistent workgroups with the channel tile's weight fragments resident
 *                   in LDS (csrc/conv_stream_lds.inc.h); tile_p = 1: four waves per workgroup, 2 (64 <= K / 32 * tile_c, K / 32 >= 8, tile_c in {4, 6, 8}):
 *                   eight waves behind the same LDS copy (csrc/conv_stream_lds_w8.hip) — same result bit for bit.
 *                   tile_k = 2 / 8 (fp16; CONV1X1 with direct / up-sampled sources and CONV3X3S2; tile_c in {4, 6, 8}, tile_p in {1, 2}, tile_k = 2 also
 *                   (4, 4)): the four waves of a workgroup share each k-step's weight fragments through LDS — 2: register -> LDS copy and a barrier per
 *                   k-step; 8: the fragments arrive by DMA (buffer load with LDS destination) in stages of two k-steps through a ring of four slots, three
 *                   stages ahead, one barrier per stage (csrc/conv_mfma_dma.hip: the K-heavy layers of the 40 x 40 / 20 x 20 maps of s and m).
 * MAF_OP_CONV3X3S2  replaces rbr_reparam / ConvWrapper.block.conv stride-2 convs.  src[0] is the
 *                   2H x 2W input (Hin, Win below); w packed per tap.
 *                   Twin launch (CONV1X1 with one direct / pooled source, CONV3X3S2; tile_k 0 / 1 / 2 / 4 / 8): aux[0] != NULL runs a SECOND conv of
 *                   identical shape, strides and tiles as blockIdx.y = 1 of the same grid — aux = {src, w, bias, out} of the second conv
 *                   (the two side ConvWrappers of a MAFPN level, configs/yaml/MAF-YOLO-n.yaml nodes 23 / 24 and 27 / 28).
 *                   tile_k = 6 (fp16; (Cin, Cout) = (48, 48), (48, 64), (64, 64)): persistent workgroups with all weight fragments and the
 *                   input patch of a 4 x 16 output tile in LDS (csrc/conv3s2_lds.hip); w = record of maf_conv3s2_lds_record_bytes(Cin, Cout)
 *                   bytes (maf-yolo_amd/pack.py:pack_conv3x3_lds: fragments + bias), bias unused, tile_c = workgroups / 64 (0 = 256).
 *                   With nc = C1 > 0 ((Cin, Cout, C1) = (48, 48, 48) or (64, 64, 64), even Hin / Win) the launch is a whole MPRep (common.py:776-792,
 *                   cat(conv1(MaxPool2d(2, 2)(x)), conv2(x))): the 2 x 2 windows of a tile's pixels lie inside its staged patch, so the pooled
 *                   1x1 + SiLU branch is taken from LDS and its C1 channels go to `out` at channel offset reg_stride (beside the conv's
 *                   out_coff .. + Cout); w = record of maf_mprep_lds_record_bytes(Cin, Cout, C1) bytes (pack.py:pack_mprep_lds).
 *                   tile_k = 7 (fp16; (Cin, Cout) = (128, 128), (96, 96), (96, 64), (64, 64)): one workgroup per CU whose waves keep ALL weight
 *                   fragments in registers, input patches of 4 x 8 output tiles by DMA, double-buffered (csrc/conv3s2_wreg.hip); w = record of
 *                   maf_conv3s2_wreg_record_bytes(Cin, Cout) bytes (pack.py:pack_conv3x3_wreg), bias unused, tile_c = workgroups per conv / 32
 *                   (0 = 256 / convs); a twin launch passes aux = {src, record, -, out} of the second conv.  With nc = C1 = 96 ((96, 96), no
 *                   twin, even Hin / Win, reg_stride + nc = out_coff) the launch is a whole MPRep as for tile_k = 6: the 2 x 2 window of an output
 *                   pixel is taps (1,1) (1,2) (2,1) (2,2) of its 3 x 3 window, so the pooled branch's operand is the maximum of four fragments the
 *                   conv reads anyway; w = record of maf_mprep_wreg_record_bytes(Cin, Cout, C1) bytes (pack.py:pack_mprep_wreg).
 * MAF_OP_CONV3X3S2_DGRAD  backward of the above w.r.t. its input (autograd of common.py:219-224 / :44-47 in Trainer.train_in_steps,
 *                   yolov6/core/engine.py:164): src[0] = dY [B,Hin,Win,Cin] (Cin = the forward conv's OUTPUT channels, Hin x Win its output
 *                   grid), out = dX [B,H,W,Cout] (Cout = the forward conv's input channels, H x W its input grid); w = the forward weight
 *                   with the channel axes swapped, packed per tap like CONV3X3S2's; bias = zeros; act = NONE; tile_p in {1,2}, tile_c in {2,4,8}.
 * MAF_OP_DWCONV     replaces DilatedReparamBlock.lk_origin after merge (common.py:3025,3033-3051).
 *                   w = [k*k][C] of the activation dtype.  tile_p / tile_c / tile_k optionally fix the workgroup tile
 *                   (rows, cols, channels per block); 0 = built-in cost model.  tile_p = -1 (fp16) selects the matrix-core
 *                   variant (csrc/dwconv_mfma.hip), whose operand is aux[0] = the Toeplitz table [C/32][8][k][parts][16][8] f16
 *                   (maf-yolo_amd/pack.py:pack_dw_toeplitz).  The other fp16 variants (same result, same operands unless noted):
 *                   tile_p = -2  v_dot2_f32_f16 over tap pairs of a pair-interleaved halo tile (csrc/dwconv_dot2.hip): tile_c = tile columns
 *                                (multiple of 8), tile_k = tile rows * 256 + channels per block (multiple of 8, <= 64);
 *                   tile_p = -3  a wave per 8-channel group, halo plane by DMA, weights as scalar operands of v_fma_mix_f32 (csrc/dwconv_sw.hip):
 *                                tile_c = tile columns (multiple of 4), tile_k = tile rows * 256 + waves per workgroup (1..8);
 *                   tile_p = -4  the same work split on v_dot2c_f32_f16 with scalar weight PAIRS over an input stored as pixel pairs
 *                                (csrc/dwconv_p2.hip): src[0].mode = MAF_SRC_PAIRS (written by the CONV1X1 in front with out_pairs = 1), even W,
 *                                aux[1] = weight pairs [C/8][k][2][2][(k+1)/2][4] dwords (pack.py:pack_dw_pairs); tile_c / tile_k as for -3.
 *                   Cout = 2 Cin runs two filters per input channel (output channel c reads input channel c mod Cin: the head's cls / reg pair).
 * MAF_OP_SPPF_POOL  replaces SPPF.m x3 (common.py:121-129): src[0] = x (slice 0 of the 4c_ buffer),
 *                   out/out_coff = slice 1; slices 2 and 3 follow at +C each.
 * MAF_OP_BOTTLENECK replaces one DepthBottleneckUni in deploy form (common.py:918-927: 1x1 c->3c + SiLU, depth-wise k x k + SiLU,
 *                   1x1 3c->c + SiLU) in one launch.  w = tile_k block records of maf_bottleneck_record_bytes() bytes, one per
 *                   32 mid channels: W1 fragments [2][S1][64][8] f16 | b1 [32] f32 | Toeplitz table of the depth-wise filter
 *                   [8][k][parts][16][8] f16 | W2 fragments [CT2][64][8] f16 | bdw [32] f32 (maf-yolo_amd/pack.py:
 *                   pack_bottleneck); bias = b2 fp32 padded to 16*CT2.  fp16 only, Cin = Cout = c <= 64, act = SiLU.
 *                   nc = C3 > 0 (where maf_bottleneck_tail_supported(k, c, nsrc, C3)): the launch also applies the 1x1 conv + SiLU that closes the
 *                   surrounding RepHDW block (common.py:944-946: conv2(torch.cat(y, 1)), y = [x1, x2, block outputs]) to its tile before anything is stored —
 *                   the LAST bottleneck of a block: src[1 .. nsrc-1] = the concat slots in front of this bottleneck's input (c channels each, direct),
 *                   src[0] = its input, then its own result from registers; aux[0] = record of maf_bottleneck_tail_record_bytes(c, nsrc, C3) bytes
 *                   (maf-yolo_amd/pack.py:pack_bottleneck_tail); out / out_stride / out_coff = the CLOSING conv's output (C3 channels) — the
 *                   bottleneck's own output is never written.
 * MAF_OP_CONV1DW    conv1 -> conv2 -> act of DepthBottleneckUni (common.py:905-909) for any width: Cin = c, Cout = 3c, ksize = k;
 *                   w = ceil(3c/32) block records of maf_conv1dw_record_bytes(k, c) bytes (W1 fragments [2][S1][64][8] f16 | b1 [32]
 *                   f32 | Toeplitz table [8][k][parts][16][8] f16 | bdw [32] f32; maf-yolo_amd/pack.py:pack_conv1dw); fp16, act = SiLU.
 * MAF_OP_STEM2      replaces backbone.0 AND backbone.1 (two RepVGGBlocks in deploy form: 3x3 s2 conv + ReLU each, common.py:216-217) in one
 *                   launch.  src[0].ptr = image [B,3,Hin,Win] NCHW of in_dtype (u8: /255 folded); H, W = the 1/4-resolution grid; Cin = 3,
 *                   ksize = C0 (channels of backbone.0), Cout = C1: (24, 48) or (32, 64); nc = C3: 0, or C1 to also apply the 1x1 conv + SiLU
 *                   that opens the next RepHDW block (backbone.2.conv1, common.py:898-946) before anything is written — out then receives
 *                   C3 channels; w = record of maf_stem2_record_bytes(C0, C1, C3) bytes (maf-yolo_amd/pack.py:pack_stem2); fp16 engine only;
 *                   tile_p = tile rows (0 / 8, or 4), tile_k = workgroups (0 = default, persistent).  aux[0] != NULL (needs nc = C1): RepHDW
 *                   splits that tensor in two (x.split((c_, c_), 1), common.py:940) — channels C3/2.. then go to aux[0], a tensor of its own with
 *                   pixel stride reg_stride (elements, a multiple of 8), and out receives channels 0..C3/2-1: a reader of ONE half then
 *                   fetches whole cache lines of what it uses instead of every line of an interleaved buffer.
 * MAF_OP_HEADTAIL   replaces, for ONE level, cls_conv_s + cls_pred + sigmoid and reg_conv_s + reg_pred (Head_DepthUni, common.py:1288-1336:
 *                   Conv.forward_fuse, nn.Conv2d) and that level's share of the Detect_yaml eval branch (yolo.py:355-396) in one launch.
 *                   src[0] / src[1] = inputs of cls_conv_s / reg_conv_s (C = Cin = head width: 64, 128, 192 — weights LDS-resident — or 256, 384 — weights streamed from L2); w / aux[0] = weight
 *                   records of the cls / reg branch, maf_head_tail_record_bytes(Cin) bytes each (maf-yolo_amd/pack.py:pack_head_tail);
 *                   out = pred fp32 [B, A, 85] (supplied per run like DECODE's); Hin = first anchor of the level, Win = A (anchors
 *                   per image), lvl_stride[0] = stride; nc = 80, reg_max = 16; fp16 only.  tile_k = units per wave (0 = auto).
 * MAF_OP_DECODE     replaces Detect_yaml.forward eval branch (yolov6/models/yolo.py:355-396).
 *                   src[l] (l<3): ptr = cls fp32 [B,HW_l,src[l].stride] (row stride >= nc; 0 = nc: the pred conv pads nc to a multiple
 *                   of 4 channels so that any class count runs), and reg[l] = fp32 [B,HW_l,reg_stride] (both NULL: the level's rows are
 *                   written by a MAF_OP_HEADTAIL, lvl_h / lvl_w still give its size);
 *                   out = pred fp32 [B, A, 5+nc].
 */
typedef struct {
    int32_t kind, dtype, in_dtype, act;
    int32_t B, H, W;             /* output grid per image                                       */
    int32_t Hin, Win;            /* input grid (STEM, CONV3X3S2)                                */
    int32_t Cin, Cout, ksize;
    int32_t nsrc;
    maf_src_t src[4];
    void* out;
    int32_t out_stride, out_coff;
    int32_t out_f32;             /* CONV1X1: store fp32 regardless of dtype (cls_pred/reg_pred) */
    int32_t tile_p, tile_c;      /* MFMA tile: 16*tile_p pixels x 16*tile_c channels per wave   */
    int32_t tile_k;              /* convs: MAF_CONV_* / MAF_CONV3_* (0 = MAF_CONV_GENERIC; the dgrad op takes 0 / 1 only); other kinds: see above */
    const void* w;
    const float* bias;
    /* DECODE only */
    const void* reg[3];
    int32_t lvl_h[3], lvl_w[3];
    int32_t reg_stride, nc, reg_max;
    float lvl_stride[3];
    const void* aux[4];          /* DWCONV: aux[0] = Toeplitz table of the matrix-core variant (else 0)                 */
    /* engine scheduling (ignored by maf_op_launch): independent branches of the graph run on separate HIP streams */
    int32_t lane;                /* 0 = the caller's stream; 1..7 = engine-owned side streams                          */
    int32_t n_wait;              /* ops on OTHER lanes whose results this op reads (<= 8): indices into the op list     */
    int32_t wait[8];
    int32_t out_pairs;           /* CONV1X1 (fp16, tile_k = 5): store the output as pixel pairs (MAF_SRC_PAIRS) for a depth-wise consumer */
    int32_t reserved0;
} maf_op_t;

const char* maf_last_error(void);
int maf_version(void);
/* sizeof(maf_op_t) as this library was compiled: a binding checks its own struct against it at load time (a stub that is short of
 * fields would make maf_engine_create read past every element of the op array). */
int maf_op_size(void);
/* The signatures of this header as the library was compiled (csrc/abi.hip): entry i < maf_abi_count() is an exported function's name and its signature as a
 * string, one character for the return type, ':', one character per parameter — v void (return only), s const char*, p any other pointer (maf_stream_t
 * included), f float, d double, i int32_t / int, l int64_t; maf_nms_workspace_bytes is "l:iii".  The compiler derives the strings from the prototypes
 * above and below and refuses any other type, so a binding that sets its argument types from this table (maf-yolo_amd/lib.py does) follows a changed
 * prototype with the next build instead of passing shifted arguments.  Every function of this header is in the table, these three included; NULL
 * for an index out of range. */
int32_t maf_abi_count(void);
const char* maf_abi_name(int32_t i);
const char* maf_abi_signature(int32_t i);
/* Bytes of one 32-mid-channel block record of MAF_OP_BOTTLENECK for kernel size k and c = Cin = Cout channels. */
int64_t maf_bottleneck_record_bytes(int32_t k, int32_t Cin, int32_t Cout);
/* MAF_OP_BOTTLENECK with nc = C3 > 0 (the closing 1x1 of the RepHDW block behind it): bytes of aux[0]'s record for c channels per concat slot and nsrc
 * slots read from memory (0: C3 no multiple of 16 / nsrc outside 2..3), and whether the (k, c, nsrc, C3) instantiation exists. */
int64_t maf_bottleneck_tail_record_bytes(int32_t c, int32_t nsrc, int32_t C3);
int maf_bottleneck_tail_supported(int32_t k, int32_t c, int32_t nsrc, int32_t C3);
int64_t maf_conv1dw_record_bytes(int32_t k, int32_t Cin);
int64_t maf_head_tail_record_bytes(int32_t C);
int64_t maf_stem2_record_bytes(int32_t C0, int32_t C1, int32_t C3);
int64_t maf_conv3s2_lds_record_bytes(int32_t Cin, int32_t Cout);
/* ... with the pooled 1x1 branch of MPRep behind it (MAF_OP_CONV3X3S2, tile_k = 6, nc = C1; maf-yolo_amd/pack.py:pack_mprep_lds). */
int64_t maf_mprep_lds_record_bytes(int32_t Cin, int32_t Cout, int32_t C1);
/* ... and on the tile_k = 7 kernel ((96, 96, 96); 0 = no such kernel; pack.py:pack_mprep_wreg). */
int64_t maf_mprep_wreg_record_bytes(int32_t Cin, int32_t Cout, int32_t C1);
int64_t maf_conv3s2_wreg_record_bytes(int32_t Cin, int32_t Cout);   /* 0: no instantiation for this shape */
/* MAF_OP_CONV1X1 with tile_k = 5, tile_p = 1, ONE direct source, act = NONE and aux[0] = NULL takes aux[2] = half of the scratch of the training-mode BatchNorm
 * behind the conv ([reserved0 replicas][2][Cout] fp32, the layout maf_dw_branches_stats fills; reserved0 = maf_bn_replicas(Cout, R)): the conv's epilogue adds
 * the sum and the sum of squares of the outputs it stores (after their rounding to the activation dtype), and the BatchNorm call runs as
 * maf_bn_forward_ex(..., stats_ready = 1) — no statistics pass (Conv.forward in training mode, yolov6/layers/common.py:44-47: conv -> bn -> act;
 * csrc/conv_stream_lds_st.hip).  Whether the (K / 32, tile_c) instantiation exists: */
int maf_conv1x1_stats_supported(int32_t ksteps, int32_t tile_c);

/* Launch one op on `stream`. */
int maf_op_launch(const maf_op_t* op, maf_stream_t stream);

/* A plan = ordered op list (Model.forward's node loop, yolo.py:186-201, flattened to launches).  Ops carry a lane: the
 * engine launches lane-0 ops on the caller's stream and the others on its own streams, with event waits for the cross-lane
 * reads listed in `wait` (the MAFPN neck and the three heads are independent branches: small-map layers overlap big ones);
 * all lanes fork from and join the caller's stream inside every run call, so the call keeps single-stream semantics. */
typedef struct maf_engine maf_engine_t;
int maf_engine_create(const maf_op_t* ops, int32_t n_ops, maf_engine_t** out);
int maf_engine_num_ops(const maf_engine_t* e);
/* image / pred override the STEM input and DECODE output pointers when non-NULL. */
int maf_engine_run(maf_engine_t* e, const void* image, void* pred, maf_stream_t stream);
/* maf_engine_run + the candidate filter of non_max_suppression inside the forward: the head-tail kernels (MAF_OP_HEADTAIL) append every
 * (box, class) whose score exceeds `conf_thres` to the candidate lists of `nms_workspace` (a buffer of maf_nms_workspace_bytes(B, A, 80) bytes; its
 * counters are reset here), so that a following maf_nms_ex(pred, ..., conf_thres, ..., multi_label = 1, workspace = nms_workspace, flags |
 * MAF_NMS_PRECOLLECTED) skips its own pass over the prediction (yolov6/utils/nms.py:48,69,75-77 folded into yolov6/models/yolo.py:355-396).
 * Needs every level's tail to be a MAF_OP_HEADTAIL (MAF_E_UNSUPPORTED otherwise), H * W of every level a multiple of 16, 0 <= conf_thres < 1. */
int maf_engine_run_filtered(maf_engine_t* e, const void* image, void* pred, maf_stream_t stream, void* nms_workspace, double conf_thres);
/* Same launches replayed from a hipGraph captured on first use (bs=1 latency path). Pointers are
 * frozen at capture time: image/pred must be the same on every call. */
int maf_engine_run_graph(maf_engine_t* e, const void* image, void* pred, maf_stream_t stream);
/* One forward with a HIP event pair around every op; ms_per_op (HOST float[n_ops]) receives each
 * op's duration.  Synchronises the stream.  Used by bench.py for the per-kernel roofline. */
int maf_engine_run_timed(maf_engine_t* e, const void* image, void* pred, maf_stream_t stream, float* ms_per_op);
void maf_engine_destroy(maf_engine_t* e);

/*
 * non_max_suppression (yolov6/utils/nms.py:31-105) for a whole batch in two launches.
 *   pred      fp32 [B,N,5+nc]
 *   classes   optional device int32[n_classes] filter (nms.py:83-84), NULL = none
 *   workspace device scratch of maf_nms_workspace_bytes(B,N,nc) bytes
 *   out_rows  fp32 [B,max_det,6] (x1,y1,x2,y2,conf,cls) in descending conf order
 *   out_idx   int64 [B,max_det]  flat candidate index: box*nc+cls (multi_label) or box
 *   out_count int32 [B]
 * Rules kept from the reference: strict '>' on conf_thres in fp32 (nms.py:48,76,80); candidate order
 * = row-major (box,class) (nms.py:76); conf = cls*obj (nms.py:69); boxes offset by cls*4096 unless
 * agnostic (nms.py:94-95); > 30000 candidates -> top 30000 by score (nms.py:90-91); keep <= max_det
 * (nms.py:97-98); greedy rule of torchvision.ops.nms (suppress when IoU > iou_thres, ties broken by
 * lower candidate index, the fp32 IoU compared with iou_thres in double as torchvision's CPU kernel
 * does).  conf_thres is applied in fp32 (what `tensor > python_float` does).  The 10 s wall-clock
 * break (nms.py:101-103) is dropped.  max_det <= 1024.
 */
enum { MAF_NMS_FLOAT_THRESHOLD = 1, MAF_NMS_SINGLE_LAUNCH = 2, MAF_NMS_PRECOLLECTED = 4, MAF_NMS_MATRIX = 8 };
enum { MAF_NMS_CNT_STRIDE = 64 };       /* ints between the candidate counters of two images in the NMS workspace (one 256-byte line each) */
/* maf_nms_ex flags.
 * MAF_NMS_FLOAT_THRESHOLD: compare the fp32 IoU with fl32(iou_thres) — torchvision's CUDA kernel (`float iou_threshold`), which is what
 *   yolov6/utils/nms.py:96 reaches when the reference runs on a GPU — instead of with the double (its CPU kernel, the default here and the rule of
 *   the oracle and of the golden fixtures).  The results differ only for a pair whose fp32 IoU equals fl32(iou_thres) exactly where
 *   fl32(iou_thres) > iou_thres (0.6, 0.7, ...).
 * MAF_NMS_SINGLE_LAUNCH: the whole call is ONE kernel (csrc/nms.hip:nms_single_kernel: every workgroup collects candidates, the last one to
 *   finish an image sorts and selects them) instead of seven; same results bit for bit.  Measured on configs[4] (m, bs 1): 0.29 ms against
 *   0.20 ms for the seven launches (whose pair-matrix kernel uses the whole chip) — available, not the default.
 * MAF_NMS_MATRIX: images on the all-pairs path (<= 4096 candidates, no per-class split) build the n x n suppression bit matrix on the whole chip and scan its rows
 *   (rounds 2-5's form, two launches) instead of the kept-list scan (one workgroup per image tests every block of 64 sorted candidates against the boxes kept so
 *   far only; the default since round 6).  Same survivors bit for bit; kept for A/B.
 * MAF_NMS_PRECOLLECTED: the candidate lists of `workspace` (counters + keys) are already there — written by the forward pass that produced `pred`
 *   (maf_engine_run_filtered: the head-tail kernels test the scores they have just computed against the same conf_thres) — so the call skips its
 *   counter reset and its pass over the prediction tensor.  Only for multi_label with nc > 1, no class filter, conf_thres < 1. */
int64_t maf_nms_workspace_bytes(int32_t B, int32_t N, int32_t nc);
int maf_nms(const float* pred, int32_t B, int32_t N, int32_t nc, double conf_thres, double iou_thres,
            const int32_t* classes, int32_t n_classes, int32_t agnostic, int32_t multi_label,
            int32_t max_det, void* workspace, int64_t workspace_bytes,
            float* out_rows, int64_t* out_idx, int32_t* out_count, maf_stream_t stream);
int maf_nms_ex(const float* pred, int32_t B, int32_t N, int32_t nc, double conf_thres, double iou_thres,
               const int32_t* classes, int32_t n_classes, int32_t agnostic, int32_t multi_label,
               int32_t max_det, void* workspace, int64_t workspace_bytes,
               float* out_rows, int64_t* out_idx, int32_t* out_count, int32_t flags, maf_stream_t stream);

/*
 * Training-side entry points.  The train-form graph keeps conv and BatchNorm apart
 * (yolov6/layers/common.py:46-47, 219-224, 3024-3031), so the convs run through maf_op_launch with a zero bias and
 * act = none; their backward needs:
 *   maf_pack_w1x1   fp32 weight [Cout][Cin] of nn.Conv2d(k=1) -> the fragment-packed operand of MAF_OP_CONV1X1 in `dtype`;
 *                   transpose = 1 packs W^T, which turns the same kernel into the data gradient dX = dY * W.
 *   maf_pack_dw     fp32 depth-wise weight [C][k*k] -> [k*k][C] in `dtype`; flip = 1 gives the data-gradient kernel.
 *   maf_dw_wgrad    dW[c][ky][kx] += sum over pixels of dY * shifted X.  dw = `replicas` zeroed copies [replicas][C][k*k] fp32: the
 *                   workgroups spread their atomics over the copies (atomics on one cache line serialise), the caller sums them.
 *   maf_conv1x1_wgrad  dW[co][ci] += sum over the M = B*H*W pixels of dY[m][co] * X[m][ci]  (fp16 NHWC views, fp32 result
 *                   accumulated with atomics: dw must be zeroed by the caller) — pixel chunks per workgroup, tiles transposed
 *                   through LDS, MFMA; replaces the TN GEMM with a tiny output and a huge reduction.
 */
int64_t maf_pack_w1x1_bytes(int32_t Cout, int32_t Cin, int32_t transpose, int32_t dtype, int32_t tile_c);
int maf_pack_w1x1(const float* w, int32_t Cout, int32_t Cin, int32_t transpose, int32_t dtype, int32_t tile_c, void* out, maf_stream_t stream);
int maf_pack_dw(const float* w, int32_t C, int32_t k, int32_t flip, int32_t dtype, void* out, maf_stream_t stream);
/* Task-aligned label assignment on RAGGED targets, no host round trip.
 *   maf_tal_targets  replaces ComputeLoss.preprocess (yolov6/models/loss.py:179-188: python lists + targets.cpu().numpy()):
 *                    targets [T][6] = (image, class, cx, cy, w, h) normalised -> gts [T][5] = (label, x1, y1, x2, y2 in pixels) grouped by
 *                    image in their original order, gt_image [T], offsets [B+1] = first row of every image.  Rows whose image id is
 *                    outside [0, B) are dropped (offsets[B] rows are valid).  T <= 16384, B <= 4096.
 *   maf_tal_assign   replaces TaskAlignedAssigner.forward (yolov6/assigners/tal_assigner.py:21-151, assigner_utils.py:25-89) as
 *                    ComputeLoss calls it (loss.py:96-103).  pd_scores [B,A,nc] (sigmoid outputs, score_dtype MAF_F16 / MAF_F32),
 *                    pd_bboxes [B,A,4] xyxy pixels fp32, cand_scratch: T*topk int32.  Anchors: n_levels <= 4 grids, level_hw [n_levels][2]
 *                    (host ints, rows x columns), level_stride [n_levels] (host floats), row-major per level, levels concatenated;
 *                    anchor_points [A,2] (device) = (cell + cell_offset) * stride as generate_anchors builds them.  out_gt [B,A] = row of
 *                    the assigned box or -1 (background), out_norm [B,A] = the normalised alignment metric that scales the one-hot
 *                    score target (tal_assigner.py:66-71).  A <= 8400; at most 8400 boxes per image are considered. */
int maf_tal_targets(const float* targets, int32_t T, int32_t B, float img_size, float* gts, int32_t* gt_image, int32_t* offsets, maf_stream_t stream);
int maf_tal_assign(const void* pd_scores, int32_t score_dtype, const float* pd_bboxes, const float* anchor_points, const float* gts,
                   const int32_t* gt_image, const int32_t* offsets, int32_t T, int32_t B, int32_t A, int32_t nc, int32_t topk,
                   float alpha, float beta, float eps, int32_t n_levels, const int32_t* level_hw, const float* level_stride, float cell_offset,
                   int32_t* cand_scratch, int32_t* out_gt, float* out_norm, maf_stream_t stream);
/* The warm-up assigner of ComputeLoss (epoch < warmup_epoch, loss.py:83-91) — replaces ATSSAssigner.forward (yolov6/assigners/atss_assigner.py:17-161,
 * iou2d_calculator.py:63-246, assigner_utils.py:4-66) on the same ragged targets and with the same outputs as maf_tal_assign:
 * out_norm = IoU of the predicted box with the assigned box (the soft label, atss_assigner.py:80-84).  topk = 9 nearest anchors per
 * level, cell_size = 5 (side of the square anchor boxes in strides, anchor_generator.py:29), cand_scratch: T * n_levels * topk int32;
 * every level needs at least 3 x 3 anchors (the reference raises below 9 anchors on a level); box centres are expected inside the image. */
int maf_atss_assign(const float* pd_bboxes, const float* anchor_points, const float* gts, const int32_t* gt_image, const int32_t* offsets,
                    int32_t T, int32_t B, int32_t A, int32_t topk, int32_t n_levels, const int32_t* level_hw, const float* level_stride,
                    float cell_offset, float cell_size, int32_t* cand_scratch, int32_t* out_gt, float* out_norm, maf_stream_t stream);
/* The loss terms of ComputeLoss (yolov6/models/loss.py:56-267, task-aligned branch) from the assigner's two arrays; head outputs in
 * `dtype` (MAF_F16 under autocast, or MAF_F32); reg_max must be 16; anchor_strides [A] = stride of every anchor.
 *   maf_loss_decode  bbox_decode (:190-193) * stride: pred_distri [B,A,4*17] logits -> out_boxes [B,A,4] xyxy pixels fp32.
 *   maf_loss_terms   VarifocalLoss (:196-206) over all scores + GIoU (figure_iou.py) and DFL (:209-267) over the foreground anchors.
 *     forward form   (upstream, grad_* NULL): out[5] (device) = weighted total, w_iou*iou, w_dfl*dfl, w_cls*cls (the order of the
 *                    reference's loss items), target-score sum; partials = scratch of maf_loss_partial_rows(B,A,nc) float4 rows.
 *     gradient form  upstream = device scalar d(objective)/d(total); out = what the forward form wrote; grad_scores / grad_distri
 *                    (shape and dtype of the inputs) receive d(objective)/d(input). */
int64_t maf_loss_partial_rows(int32_t B, int32_t A, int32_t nc);
int maf_loss_decode(const void* pred_distri, int32_t dtype, const float* anchor_points, const float* anchor_strides, int32_t B, int32_t A,
                    int32_t reg_max, float* out_boxes, maf_stream_t stream);
int maf_loss_terms(const void* pred_scores, const void* pred_distri, int32_t dtype, const float* anchor_points, const float* anchor_strides,
                   const float* gts, const int32_t* assigned_gt, const float* norm, int32_t B, int32_t A, int32_t nc, int32_t reg_max,
                   float w_cls, float w_iou, float w_dfl, float* partials, float* out, const float* upstream, void* grad_scores,
                   void* grad_distri, maf_stream_t stream);

/* BatchNorm2d in training mode fused with the activation behind it (Conv.forward = act(bn(conv(x))), common.py:46-47), NHWC views.
 *   maf_bn_forward   batch statistics -> save_mean / save_rstd (+ running stats with torch's momentum rule, unbiased variance, and
 *                    the int64 num_batches_tracked counter += 1; each may be NULL) and y = act(xhat*gamma + beta); two launches (statistics, apply).
 *                    The statistics launch accumulates {sum x, sum (x - p)^2} about a per-channel pivot p that both launches read from x (csrc/bn_act.hip);
 *                    the apply pass re-reads those pixels in every workgroup, so y MUST NOT alias x (refused).
 *   maf_bn_backward  dz = gradient w.r.t. the activation output; recomputes u from x; dx, dgamma, dbeta; two launches.
 *   residual         (may be NULL) a tensor like y added BEFORE the activation: y = act(xhat*gamma + beta + residual) — the branch sums of
 *                    RepVGGBlock (common.py:224) and DilatedReparamBlock (:3028-3031) without their own pass.  Backward needs it only when the
 *                    activation does (ReLU): then dres receives dz * act'(u); without an activation the residual's gradient IS dz (pass NULL).
 *   part             fp32 scratch of TWO halves [2][R][2][roundup(C,256)], zeroed ONCE by the caller: a call accumulates its partial sums
 *                    into half `phase` (R replicas spread the atomics) and clears half 1 - phase — the one the previous call on the stream
 *                    used — so one buffer per stream serves all BatchNorms of a step when the caller alternates phase = 0, 1, 0, ... */
int maf_bn_forward(const void* x, int32_t x_stride, int32_t M, int32_t C, int32_t dtype, const float* gamma, const float* beta,
                   float eps, float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked, int32_t act, void* y,
                   int32_t y_stride, float* save_mean, float* save_rstd, float* part, int32_t R, int32_t phase, const void* residual, int32_t res_stride,
                   maf_stream_t stream);
int maf_bn_backward(const void* x, int32_t x_stride, const void* dz, int32_t dz_stride, int32_t M, int32_t C, int32_t dtype,
                    const float* gamma, const float* beta, const float* save_mean, const float* save_rstd, int32_t act,
                    void* dx, int32_t dx_stride, float* dgamma, float* dbeta, float* part, int32_t R, int32_t phase,
                    const void* residual, int32_t res_stride, void* dres, int32_t dres_stride, maf_stream_t stream);
/* The parallel depth-wise branches of a train-form DilatedReparamBlock (yolov6/layers/common.py:3024-3031: lk_origin(x) and dil_conv_k*(x), NB
 * depth-wise "same" convolutions of ONE input with kernel sizes 3, 3, 1 / 5, 3, 1 / 7, 5, 3 / 9, 7, 5, 3 for k0 = 3 / 5 / 7 / 9 — the 1 x 1 branch is a
 * per-channel scale) in one launch per direction, NHWC, no bias, no activation (a BatchNorm follows each):
 *   dgrad = 0   dst[j] = DW(src[0], w[j]), j < nb            (the input is staged once)
 *   dgrad = 1   dst[0] = sum_j DW(src[j], w[j])             (w[j] = the flipped filters; the sum is kept in fp32 registers and written once)
 * (k0, nb) in {(3, 3), (5, 3), (7, 3), (9, 4)}; w[j]: [k_j * k_j][C] in `dtype` (maf_pack_dw); strides in elements, multiples of the 16-byte
 * channel group; src / dst arrays hold 1 / nb (forward) or nb / 1 (data gradient) entries. */
/* Forward of maf_dw_branches + the BatchNorm statistics of every branch: stats[j] (may be NULL per branch) = the half of the `part` scratch that the
 * maf_bn_forward_ex(..., stats_ready = 1) call of branch j's BatchNorm will read, [replicas][2][C] fp32, zero on entry; the kernel adds the sum and
 * the sum of squares of the (rounded) outputs it stores, spread over `replicas` = maf_bn_replicas(C, R) copies. */
int maf_dw_branches_stats(const void* const* src, const int32_t* src_stride, void* const* dst, const int32_t* dst_stride, const void* const* w,
                          int32_t nb, int32_t k0, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, float* const* stats, int32_t replicas, maf_stream_t stream);
int maf_dw_branches(const void* const* src, const int32_t* src_stride, void* const* dst, const int32_t* dst_stride, const void* const* w,
                    int32_t nb, int32_t k0, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, int32_t dgrad, maf_stream_t stream);
/* maf_bn_forward with stats_ready != 0: half `phase` of `part` already holds this call's {sum x, sum x^2} — accumulated by the kernel that produced x
 * (maf_dw_branches_stats) into replicas [0, maf_bn_replicas(C, R)) — and the statistics launch is skipped: apply only. */
int maf_bn_forward_ex(const void* x, int32_t x_stride, int32_t M, int32_t C, int32_t dtype, const float* gamma, const float* beta,
                      float eps, float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked, int32_t act, void* y,
                      int32_t y_stride, float* save_mean, float* save_rstd, float* part, int32_t R, int32_t phase, const void* residual, int32_t res_stride,
                      int32_t stats_ready, maf_stream_t stream);
int32_t maf_bn_replicas(int32_t C, int32_t R);
/* The statistics pass alone, about NO pivot (half `phase` of `part` += {sum x, sum x^2}, what maf_bn_forward_ex(stats_ready = 1) and maf_bn_sum_forward
 * expect — unlike maf_bn_forward's own launch, whose second sum is sum (x - p)^2; nothing is cleared).  Raw sums lose digits as |mean| / std grows (fp32 rows of
 * 3200 x 576 at |mean| / std = 32: save_rstd 2.4e-4 off fp64). */
int maf_bn_stats(const void* x, int32_t x_stride, int32_t M, int32_t C, int32_t dtype, float* part, int32_t R, int32_t phase, maf_stream_t stream);
/* The SUM of the nb (2..4) training-mode BatchNorm2d of a DilatedReparamBlock (common.py:3024-3031: origin_bn(lk_origin(x)) + sum_j dil_bn_j(dil_conv_j(x)),
 * no activation; act = MAF_ACT_RELU: RepVGGBlock's ReLU(BN(3x3 s2) + BN(1x1 s2)), common.py:224 — the backward recomputes the sum for the ReLU's mask)
 * as one apply pass per direction (csrc/bn_sum.hip):
 *   maf_bn_sum_forward   out = sum_j BN_j(z_j).  part[j] = branch j's own scratch ([2][R][2][roundup(C,256)], the layout of maf_bn_forward), whose half
 *                        phase[j] ALREADY holds {sum z_j, sum z_j^2} (maf_dw_branches_stats / maf_bn_stats); save_mean / save_rstd / running statistics /
 *                        num_batches_tracked per branch as in maf_bn_forward; the other half of every scratch is cleared.
 *   maf_bn_sum_backward  dy = gradient of the sum (the same for every branch): one statistics launch ({sum dy, sum dy xhat_j}), one apply launch writing
 *                        every dz_j; dgamma_j / dbeta_j written, or added when accumulate_affine != 0.  bpart = [2][R][1 + nb][roundup(C,256)] fp32, zeroed
 *                        once by the caller, halves alternating call by call (phase) like maf_bn_backward's scratch.
 * Both directions take the same (nb, C): C <= 4096 (MAF_E_ARG beyond) and (2 + 5 nb) * C * 4 bytes <= 160 KiB, the backward apply pass's LDS — C <= 3412 / 2408 /
 * 1860 for nb 2 / 3 / 4 (MAF_E_UNSUPPORTED beyond: nothing is launched, no buffer is touched). */
int maf_bn_sum_forward(const void* const* z, const int32_t* z_stride, int32_t nb, int32_t M, int32_t C, int32_t dtype,
                       const float* const* gamma, const float* const* beta, float eps, float momentum,
                       float* const* running_mean, float* const* running_var, int64_t* const* num_batches_tracked,
                       void* out, int32_t out_stride, float* const* save_mean, float* const* save_rstd,
                       float* const* part, int32_t R, const int32_t* phase, int32_t act, maf_stream_t stream);
/* maf_bn_sum_forward that ALSO accumulates the statistics of the values it stores for the training-mode BatchNorm that normalises `out` next (UniRepLKNetBlock.norm behind
 * the DilatedReparamBlock, yolov6/layers/common.py:3053-3083): half next_phase of next_part ([2][next_R][2][roundup(C,256)], that BatchNorm's own scratch) += {sum out,
 * sum out^2}; its call is then the apply pass alone (maf_bn_forward_ex, statistics ready).  next_part = NULL: maf_bn_sum_forward. */
int maf_bn_sum_forward_stats(const void* const* z, const int32_t* z_stride, int32_t nb, int32_t M, int32_t C, int32_t dtype,
                             const float* const* gamma, const float* const* beta, float eps, float momentum,
                             float* const* running_mean, float* const* running_var, int64_t* const* num_batches_tracked,
                             void* out, int32_t out_stride, float* const* save_mean, float* const* save_rstd,
                             float* const* part, int32_t R, const int32_t* phase, int32_t act,
                             float* next_part, int32_t next_R, int32_t next_phase, maf_stream_t stream);
int maf_bn_sum_backward(const void* dy, int32_t dy_stride, const void* const* z, const int32_t* z_stride, int32_t nb, int32_t M, int32_t C, int32_t dtype,
                        const float* const* gamma, const float* const* beta, const float* const* save_mean, const float* const* save_rstd,
                        void* const* dz, const int32_t* dz_stride, float* const* dgamma, float* const* dbeta, int32_t accumulate_affine,
                        float* bpart, int32_t R, int32_t phase, int32_t act, maf_stream_t stream);
/* maf_bn_backward with accumulate_affine != 0: dgamma / dbeta are ADDED to what the buffers hold — the slices of a gradient-exchange bucket
 * (maf_yolo_amd/exchange.py: `p.grad` of the BatchNorm affine parameters is a view of a flat fp32 bucket; the reference accumulates them with
 * AccumulateGrad, i.e. 280 one-line add kernels per step of MAF-YOLO-n, yolov6/core/engine.py:164). */
int maf_bn_backward_acc(const void* x, int32_t x_stride, const void* dz, int32_t dz_stride, int32_t M, int32_t C, int32_t dtype,
                        const float* gamma, const float* beta, const float* save_mean, const float* save_rstd, int32_t act,
                        void* dx, int32_t dx_stride, float* dgamma, float* dbeta, float* part, int32_t R, int32_t phase,
                        const void* residual, int32_t res_stride, void* dres, int32_t dres_stride, int32_t accumulate_affine, maf_stream_t stream);
/* Bit-reproducible BatchNorm statistics (a test / debugging mode, process-wide, one stream at a time): the statistics kernels of maf_bn_forward /
 * maf_bn_backward write per-workgroup sums with plain stores and a third launch adds them in a fixed order, instead of fp32 atomics whose order
 * changes from run to run.  With it two forward passes of the train-form graph are bit-identical (torch.use_deterministic_algorithms' role). */
int maf_set_deterministic(int32_t on);
int maf_conv1x1_wgrad(const void* x, int32_t x_stride, const void* dy, int32_t dy_stride, int32_t M, int32_t Cin, int32_t Cout,
                      int32_t dtype, float* dw, maf_stream_t stream);
/* General form: dW (fp32, accumulated into) of a conv with k = 1 (stride 1 / 2, pad 0) or k = 3 (stride 2, pad 1) — RepVGGBlock.rbr_dense /
 * rbr_1x1 (common.py:202-203), ConvWrapper (:76-83): x [B,Hs,Ws,Cin], dy [B,Ho,Wo,Cout], fp16 NHWC views.  The taps are gathered inside the
 * kernel (no im2col tensor); inputs wider than 256 channels run as channel chunks.
 * Layout of dW: k = 1 -> [Cout][Cin];  k = 3 -> TAP-MAJOR [3][3][Cout][Cin] (the lanes of an atomic then share a cache line). */
int maf_conv_wgrad(const void* x, int32_t x_stride, const void* dy, int32_t dy_stride, int32_t B, int32_t Ho, int32_t Wo, int32_t Hs, int32_t Ws,
                   int32_t Cin, int32_t Cout, int32_t ksize, int32_t stride, int32_t dtype, float* dw, maf_stream_t stream);
int maf_dw_wgrad(const void* x, int32_t x_stride, const void* dy, int32_t dy_stride, int32_t B, int32_t H, int32_t W, int32_t C,
                 int32_t k, int32_t dtype, float* dw, int32_t replicas, maf_stream_t stream);
/* Training-form stem (backbone.0's RepVGGBlock over the image, yolov6/layers/common.py:199-203, 219-224; Cin = 3: configs/yaml/MAF-YOLO-n.yaml:5): z3 = conv3x3 stride 2 pad 1
 * (img, w3) and z1 = conv1x1 stride 2 (img, w1) in ONE launch, no bias, no activation (csrc/stem_train.hip).  img: fp16 NHWC [B][Hin][Win] with 16-byte pixels (3 channels
 * zero-padded to 8; pixel stride img_stride halfs), w3 [Cout][3][3][3] / w1 [Cout][3] fp32 — the parameters themselves, rounded to fp16 inside as autocast does —, z3 / z1
 * dense fp16 [B][Hin/2][Win/2][Cout]. */
int maf_stem_train(const void* img, int32_t img_stride, int32_t B, int32_t Hin, int32_t Win, const float* w3, const float* w1, int32_t Cout,
                   void* z3, void* z1, maf_stream_t stream);
/* Input staging of the training step: contiguous NCHW images [B][3][H][W] (MAF_F32 or MAF_F16; the reference's `images.float() / 255`, yolov6/core/engine.py:426) -> the
 * NHWC fp16 buffer with 16-byte pixels that maf_stem_train and the stem's weight-gradient kernels read: out [B][H][W][8], channels 3..7 zero.  One pass. */
int maf_image_to_nhwc8(const void* x, int32_t dtype, int32_t B, int32_t H, int32_t W, void* out, maf_stream_t stream);
/* The 3x3 (+ second 3x3) + 1x1 branches of a train-form DilatedReparamBlock (kernel sets 3,3,1 / 5,3,1: yolov6/layers/common.py:2997-3008, 3024-3031) share their
 * input: ONE launch stages the X halo tile once and multiplies it with dYa (and dYb, may be null together with dwb) for the 3x3 gradients [C][9] and — the items of
 * the centre tap row — with dY1 for the 1x1 branch's per-channel scale gradient dw1[C].  Same contract as maf_dw_wgrad otherwise (zeroed fp32 results, `replicas` copies). */
int maf_dw_wgrad31(const void* x, int32_t x_stride, const void* dya, int32_t dya_stride, const void* dyb, int32_t dyb_stride, const void* dy1, int32_t dy1_stride,
                   int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, float* dwa, float* dwb, float* dw1, int32_t replicas, maf_stream_t stream);

/* Gradient fold of the owned gradient exchange (maf_yolo_amd/exchange.py; the reference leaves this to autograd's AccumulateGrad + the DDP
 * reducer's bucket copy, yolov6/core/engine.py:161-164): src = what a weight-gradient kernel produced, tap-major [taps][Cout_p][Cin_p] fp32 with
 * padded channel counts; dst = the parameter-shaped slice [Cout][Cin][taps] of a flat gradient bucket; accumulate != 0 adds (gradient
 * accumulation over several backward passes), 0 overwrites.  Runs on `stream` (the weight-gradient stream). */
int maf_grad_fold(const float* src, int32_t taps, int32_t Cout_p, int32_t Cin_p, float* dst, int32_t Cout, int32_t Cin, int32_t accumulate,
                  maf_stream_t stream);
/* dst[b, 2y, 2x, :] += src[b, y, x, :]: src [B,Ho,Wo,C], dst [B,2Ho,2Wo,C] NHWC with pixel strides in elements — the data gradient of RepVGGBlock's stride-2 1x1
 * branch (yolov6/layers/common.py:203, 224) added onto the 3x3 branch's data gradient in place. */
int maf_add_sub2(const void* src, int32_t src_stride, void* dst, int32_t dst_stride, int32_t B, int32_t Ho, int32_t Wo, int32_t C, int32_t dtype, maf_stream_t stream);
/* out[c] += sum over the M pixels of x[m * x_stride + c] (fp32 atomics; the caller zeroes or accumulates): the bias gradient of the head's prediction convs
 * (nn.Conv2d with bias, yolov6/layers/common.py:1304-1305).  C <= 256. */
int maf_colsum(const void* x, int32_t x_stride, int64_t M, int32_t C, int32_t dtype, float* out, maf_stream_t stream);

/* Zero `bytes` bytes at p on `stream` (hipMemsetAsync): the fp32 accumulation buffers of maf_conv_wgrad / maf_dw_wgrad when those run on a stream
 * of their own. */
int maf_zero(void* p, int64_t bytes, maf_stream_t stream);

/* MaxPool2d(k, stride, padding) of the training graph — SPPF.m (5, 1, 2; yolov6/layers/common.py:114-129) and MP (2, 2, 0; :667-673) —
 * NHWC views, fp16 / fp32, floor mode: x [B,H,W,C] -> y [B,Ho,Wo,C], Ho = floor((H + 2 pad - k) / stride) + 1.  Forward keeps the chosen
 * window element (row * k + column, first maximum in scan order like aten) as one byte per element in idx [B,Ho,Wo,C]; backward is a
 * gather over the windows that contain an input element (no atomics). */
int maf_maxpool_forward(const void* x, int32_t x_stride, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, int32_t pad,
                        int32_t dtype, void* y, int32_t y_stride, uint8_t* idx, maf_stream_t stream);
int maf_maxpool_backward(const void* dy, int32_t dy_stride, const uint8_t* idx, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k,
                         int32_t stride, int32_t pad, int32_t dtype, void* dx, int32_t dx_stride, maf_stream_t stream);
/* nn.Upsample(scale_factor=2, mode="nearest") of the training graph (the neck's two up-sampling nodes, configs/yaml/MAF-YOLO-n.yaml) on NHWC views with pixel strides
 * in elements — source and destination may be channel slices (slots of a concat buffer): y [B,2H,2W,C] from x [B,H,W,C]; backward dx = the sum of the four. */
int maf_upsample2x_forward(const void* x, int32_t x_stride, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, void* y, int32_t y_stride, maf_stream_t stream);
int maf_upsample2x_backward(const void* dy, int32_t dy_stride, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, void* dx, int32_t dx_stride, maf_stream_t stream);

/* Weight staging of a whole training step in one launch.  A descriptor transforms one fp32 weight tensor:
 *   kind 0  dense conv weight [Cout][Cin][taps] (taps = 1 or 9) -> the MFMA fragment order of maf_pack_w1x1 with tile_c = CT; K runs
 *           tap-major, every tap padded to Kp (a multiple of the k-step: 32 fp16 / 16 fp32), steps = taps * Kp / k-step for 3x3 and
 *           ceil(K / k-step) for 1x1 (then Kp = steps * k-step); transpose = 1 packs W^T (the data gradient's operand)
 *   kind 1  depth-wise kernel [C = Cout][taps = k*k] -> [k*k][C], flip = 1 reverses the taps (data gradient)
 *   kind 2  fp32 vector of Cout values -> `total` fp32 values, zero behind the Cout-th (the bias of a prediction conv padded to the conv's channel tile)
 * total = packed elements, block0 = first block of the descriptor in the flattened grid (1024 elements per block; ascending),
 * nblocks = sum of ceil(total / 1024).  The descriptor array lives in DEVICE memory. */
typedef struct maf_pack_desc {
    const void* src; void* dst;
    int64_t total;
    int32_t kind, dtype;
    int32_t Cout, Cin, taps, transpose;
    int32_t CT, steps, Kp, flip;
    int32_t block0, reserved;
} maf_pack_desc_t;
int maf_pack_batch(const maf_pack_desc_t* descs_dev, int32_t n, int32_t nblocks, maf_stream_t stream);
int32_t maf_pack_desc_size(void);

/* ModelEMA.update (yolov6/utils/ema.py:25-37: `v *= d; v += (1 - d) * msd[k].detach()` for every floating-point state_dict entry) in one
 * launch over a descriptor table in DEVICE memory: dst (the average) and src (the model) fp32, `total` elements, block0 = first block of the
 * entry in the flattened grid (1024 elements per block; ascending), nblocks = sum of ceil(total / 1024).  decay and one_minus_decay are the
 * two scalars as the reference's tensor ops see them (Python doubles rounded to fp32); the two products and the sum are rounded
 * separately, so the result is bit-identical to the reference's three element-wise ops. */
typedef struct maf_ema_desc {
    void* dst; const void* src;
    int64_t total;
    int32_t block0, reserved;
} maf_ema_desc_t;
int maf_ema_update(const maf_ema_desc_t* descs_dev, int32_t n, int32_t nblocks, float decay, float one_minus_decay, maf_stream_t stream);
int32_t maf_ema_desc_size(void);

/* The optimizer step of the train loop (yolov6/core/engine.py:375-391: `self.scaler.step(self.optimizer)`; optimizer = torch.optim.SGD(momentum, nesterov=True) over
 * the three groups of yolov6/solver/build.py:12-33) for every parameter in ONE launch over a descriptor table in DEVICE memory: param / grad / buf fp32 (buf = the
 * momentum buffer, NULL for momentum 0), `total` elements, block0 as in the EMA table above — 1024 elements per block, group = index into the per-group hyper-parameters
 * (host arrays of ngroups <= MAF_SGD_MAX_GROUPS doubles: what the framework's optimizer holds).  found_inf / grad_scale: the GradScaler's device scalars (NULL = none) —
 * found_inf == 1 skips the update, grad_scale un-scales the gradients (and they are written back un-scaled), no host round trip.  Per element, in double where the
 * framework's fused kernel computes in double (each multiply-add one fused operation, as its build contracts them):  g = g / scale;  g += wd * p;  buf = mu * buf + g;
 * g = nesterov ? g + mu * buf : buf;  p -= lr * g. */
#define MAF_SGD_MAX_GROUPS 8
typedef struct maf_sgd_desc {
    void* param; void* grad; void* buf;
    int64_t total;
    int32_t block0, group;
} maf_sgd_desc_t;
int maf_sgd_update(const maf_sgd_desc_t* descs_dev, int32_t n, int32_t nblocks, int32_t ngroups, const double* lr, const double* weight_decay, const double* momentum,
                   const int32_t* nesterov, const float* found_inf, const float* grad_scale, maf_stream_t stream);
int32_t maf_sgd_desc_size(void);

/* The inf check GradScaler.step runs over the optimizer's gradients before the step (yolov6/core/engine.py:375-391) in one launch over a table of the contiguous
 * fp32 ranges they occupy, in DEVICE memory: ptr, `total` elements, block0 = first block of the range in the flattened grid, 4096 elements per block (ascending;
 * nblocks = sum of ceil(total / 4096)).  *found_inf (a device float the caller has zeroed) becomes 1 if any element is Inf or NaN. */
typedef struct maf_range_desc {
    const void* ptr;
    int64_t total;
    int32_t block0, reserved;
} maf_range_desc_t;
int maf_nonfinite_check(const maf_range_desc_t* descs_dev, int32_t n, int32_t nblocks, float* found_inf, maf_stream_t stream);
int32_t maf_range_desc_size(void);


/* dst = [dst +] sum_i src[i] over NHWC views with pixel strides in elements (channel slices of wider buffers are fine): n = 1, accumulate = 0 is a strided copy
 * (a concat input its producer could not store in place: torch.cat of the neck, configs/yaml/MAF-YOLO-n.yaml:16-42), n = 1, accumulate = 1 an in-place add
 * (a tensor that feeds a concat AND a later block: the block's gradient added into the concat's), n = 2..4 the gradient of a tensor with several consumers
 * (what autograd's engine does with one add kernel per extra consumer).  fp16 (fp32 sums, one rounding) / fp32; C and strides in whole 16-byte groups. */
int maf_nhwc_sum(const void* const* src, const int32_t* src_stride, int32_t n, void* dst, int32_t dst_stride, int64_t M, int32_t C, int32_t dtype,
                 int32_t accumulate, maf_stream_t stream);
/* Detect_yaml.forward, TRAIN branch (yolov6/models/yolo.py:333-354) with the head's class sigmoid (yolov6/layers/common.py:1332) folded in: per level l the NHWC maps
 * cls[l] (class LOGITS, nc channels, pixel stride cls_stride[l] elements) and reg[l] (nreg = 4 * (reg_max + 1) channels) of B images with level_pixels[l] = h*w
 * pixels each become rows [a0_l, a0_l + h*w) of cls_out [B, A, nc] = sigmoid(logits) and reg_out [B, A, nreg] (A = sum of level_pixels) — the reference's
 * flatten(2).permute(0, 2, 1) + torch.cat.  f16 / f32; nc, nreg and the strides multiples of 4.  Host arrays are read at call time.
 * Backward: d logits = d_cls * y * (1 - y) (y = cls_out: what the framework's sigmoid backward computes from its saved output) and d_reg scattered back into per-level
 * NHWC gradient maps of nc_pad / nreg_pad channels (>= nc / nreg, the 16-byte group the conv kernels read; pad channels are WRITTEN as zeros).  d_cls / d_reg NULL =
 * no gradient (zeros). */
int maf_detect_join(const void* const* cls, const int32_t* cls_stride, const void* const* reg, const int32_t* reg_stride, const int32_t* level_pixels,
                    int32_t n_levels, int32_t B, int32_t nc, int32_t nreg, int32_t dtype, void* cls_out, void* reg_out, maf_stream_t stream);
int maf_detect_join_backward(const void* d_cls, const void* d_reg, const void* cls_out, const int32_t* level_pixels, int32_t n_levels, int32_t B, int32_t nc,
                             int32_t nreg, int32_t dtype, void* const* dcls, const int32_t* dcls_stride, void* const* dreg, const int32_t* dreg_stride,
                             int32_t nc_pad, int32_t nreg_pad, maf_stream_t stream);
/* `side` waits for what `main` holds now (an event record + a stream wait: the fork of a weight gradient to its own stream); join: `main` waits for `side`. */
int maf_stream_fork(maf_stream_t main, maf_stream_t side);
int maf_stream_join(maf_stream_t main, maf_stream_t side);

/* A stream restricted to the compute units of a bit mask (n_words x 32 bits; bit i = CU i in the driver's numbering): bench.py's serving loop can confine the
 * NMS of batch i (yolov6/utils/nms.py:31-105) to a slice of the chip while the forward of batch i + 1 runs on the rest.  Destroy with maf_stream_destroy. */
int maf_stream_create_masked(const uint32_t* mask_words, int32_t n_words, maf_stream_t* out);
int maf_stream_destroy(maf_stream_t s);

/*
 * Step tape: a recorded launch list of the C-ABI calls of one training step (yolov6/core/engine.py:141-167: forward, backward), replayed by ONE call.
 * The train-form graph is ~420 launches forward and ~470 backward of kernels that take 5-60 us each; issued one by one from Python autograd
 * Functions the host needs 19-27 ms per step — the step itself.  The Python side (maf_yolo_amd/tape.py) records every call of a step — entry point,
 * arguments, stream — once per (model, batch shape) while it runs the step the normal way with every buffer kept alive, and later steps replay the list:
 * the kernels, their order and their streams are exactly the recorded ones, launched eagerly (a hipGraph node costs ~1.1 us more than an eager launch
 * on this part).
 *   fn      index into the table of tape-able entry points (maf_tape_fn_id(name)); MAF_TAPE_FORK = maf_stream_fork(streams[a[0]], streams[a[1]])
 *   stream  index into the `streams` array of maf_tape_run the entry's last argument (its maf_stream_t) is taken from: 0 the main stream, 1 the weight-gradient
 *           stream, 2.. lanes (independent branches of the graph — the two branches of a detection head — recorded on streams of their own)
 *   a[]     the arguments in declaration order, one 64-bit slot each: pointers and integers as they are, a float as its 32 bits; pointer-to-array
 *           arguments point at host arrays the recorder keeps alive
 * Toggles: words that alternate from step to step (the phase of a BatchNorm scratch: which half this step accumulates into) are XOR-ed with their
 * mask by maf_tape_toggle between two runs.
 */
#define MAF_TAPE_MAX_ARGS 28
#define MAF_TAPE_FORK (-1)
typedef struct maf_tape_rec {
    int32_t fn, stream;
    uint64_t a[MAF_TAPE_MAX_ARGS];
} maf_tape_rec_t;
typedef struct maf_tape_toggle {
    void* addr; uint64_t mask; int32_t width, reserved;     /* width 4 or 8 bytes */
} maf_tape_toggle_t;
int32_t maf_tape_fn_id(const char* name);                   /* -1000: not a tape-able entry point */
int32_t maf_tape_fn_nargs(int32_t fn);
int32_t maf_tape_rec_size(void);
int maf_tape_run(const maf_tape_rec_t* recs, int32_t first, int32_t last, const maf_stream_t* streams, int32_t n_streams, int32_t* failed_at);
int maf_tape_toggle(const maf_tape_toggle_t* t, int32_t n);

/*
 * Post-NMS tail — replaces Evaler.scale_coords (yolov6/core/evaler.py:382-409, ratio_pad branch), box_convert
 * (:374-381) and the tensor part of convert_to_coco_format (:411-420) for a whole batch in one launch.
 *   rows [B,max_det,6] / count [B]   the outputs of maf_nms
 *   img_params [B][6] fp32           original h0, w0, gain applied to x, gain applied to y, pad_w, pad_h  (the reference divides
 *                                    x by gain[1] only with scale_exact, else both axes by gain[0])
 *   ids [n_ids]                      class index -> dataset category id (COCO 80 -> 91 table), may be NULL with n_ids = 0
 *   out [sum(count)][7] fp32         image index in the batch, category id, x, y, w, h (original-image pixels), score;
 *                                    rows of image b follow those of image b-1; *out_total = number of rows
 */
int maf_coco_rows(const float* rows, const int32_t* count, int32_t B, int32_t max_det, const float* img_params,
                  const int32_t* ids, int32_t n_ids, float* out, int32_t* out_total, maf_stream_t stream);

/*
 * Letterbox on the device — replaces letterbox() (yolov6/data/data_augment.py:53-82: cv2.resize INTER_LINEAR to new_unpad,
 * copyMakeBorder with a constant colour) plus the HWC -> CHW / BGR -> RGB of Inferer.precess_image (yolov6/core/inferer.py:169-179), or
 * TrainValDataset.load_image's resize plus the rect letterbox of __getitem__ (yolov6/data/datasets.py:277-300, :196-213), for a whole batch
 * in one launch.  The geometry (new_h, new_w, top, left) is computed by the caller (maf-yolo_amd/letterbox.py); the pixel rule is OpenCV's
 * uint8 INTER_LINEAR as restated in tests/letterbox_ref.py, an exact 2x shrink on both axes is its area-fast average, equal sizes a copy.
 *   imgs [B]      HOST table, one entry per frame: frame = uint8 HWC (3 channels, channel stride 1, pixel stride 3, row pitch in bytes)
 *   imgs_dev      device copy of the same table; needed only for B > MAF_LETTERBOX_KARG_MAX (smaller tables travel as kernel arguments)
 *   H, W          the common output size, positive multiples of 32; top + new_h <= H, left + new_w <= W for every frame
 *   color [3]     HOST: the border colour, in the frame's channel order (the reference's (114, 114, 114))
 *   bgr           1: frames are BGR (cv2.imread) and are swapped to RGB as precess_image's [::-1] does; 0: frames are RGB
 *   out           DEVICE, 4-byte aligned, uint8 [B, 3, H, W] (RGB planes): every byte written exactly once, border included (32-bit stores)
 *   frames        DEVICE memory; every read stays inside [row * pitch, row * pitch + 3 w) of a row < h
 * Validates everything above before touching the device.  maf_letterbox_lds_bytes: the launch's LDS size (at most 64 KiB).
 */
#define MAF_LETTERBOX_KARG_MAX 64
typedef struct {
    const uint8_t* ptr; int64_t pitch;
    int32_t h, w;                        /* source frame */
    int32_t new_h, new_w, top, left;     /* unpadded (resized) size and its offset in the output */
} maf_letterbox_image_t;
int64_t maf_letterbox_lds_bytes(const maf_letterbox_image_t* imgs, int32_t B, int32_t W);
int maf_letterbox(const maf_letterbox_image_t* imgs, const maf_letterbox_image_t* imgs_dev, int32_t B, int32_t H, int32_t W,
                  const uint8_t* color, int32_t bgr, uint8_t* out, maf_stream_t stream);

/*
 * Inferer.rescale (yolov6/core/inferer.py:181-195) and the .round() of :98, in place on the NMS result of a batch (maf_nms rows / count):
 * All three arrays are DEVICE pointers (the NMS result stays on the device).
 *   rows [B][max_det][row_stride] fp32   columns 0..3 (x1, y1, x2, y2) of the first count[b] rows of image b are rewritten
 *   params [B][5] fp32                   h0, w0 (source frame), ratio = min(H / h0, W / w0), pad_x = (W - w0 ratio) / 2, pad_y = (H - h0 ratio) / 2
 *   do_round                             1: round half to even after the clamp (torch.round)
 * (x - pad) / ratio as an IEEE fp32 divide, clamp to [0, w0] / [0, h0] — the operation order of the reference's tensor ops on the CPU.
 */
int maf_rescale_boxes(float* rows, const int32_t* count, int32_t B, int32_t max_det, int32_t row_stride, const float* params,
                      int32_t do_round, maf_stream_t stream);

/*
 * Training augmentation on the device — replaces the pixel work of TrainValDataset.__getitem__ (yolov6/data/datasets.py:
 * 147-275) for a batch; the random parameters and the labels are host bookkeeping (maf-yolo_amd/augment.py), the pixel rules are those of
 * tests/augment_ref.py, bit for bit.
 *
 * maf_augment_resize: load_image's cv2.resize INTER_LINEAR (augment mode), n frames in one launch, uint8 HWC in, uint8 HWC out.
 *   frames [n]    HOST table (validated); frames_dev: DEVICE copy of the same table, read by the kernel (always required)
 *   src           DEVICE, uint8 HWC (3 channels, pixel stride 3, row pitch src_pitch >= 3 w bytes); reads stay in [row * pitch, + 3 w) of rows < h
 *   dst           DEVICE, uint8 HWC new_h x new_w, pitch 3 new_w, no alignment needed; every byte written once; must not overlap any src
 *   The rule of maf_letterbox's resize (tests/letterbox_ref.py): INTER_LINEAR, the exact-2x area-fast average, a copy for equal sizes.
 */
typedef struct {
    const uint8_t* src; int64_t src_pitch;
    int32_t h, w;                        /* source frame */
    uint8_t* dst;
    int32_t new_h, new_w;                /* resized frame, pitch 3 new_w */
} maf_augment_frame_t;
int maf_augment_resize(const maf_augment_frame_t* frames, const maf_augment_frame_t* frames_dev, int32_t n, maf_stream_t stream);

/*
 * maf_mosaic_affine: the uint8 [B, 3, S, S] RGB batch from per-sample parameters, one launch: for every output pixel, the flip index map,
 * OpenCV's fixed-point warpAffine (INTER_LINEAR, BORDER_CONSTANT 114) of the virtual mosaic canvas — never materialised: a canvas pixel is
 * read from the tile whose rectangle holds it, 114 elsewhere — the mixup blend with a second warped canvas, uint8 BGR2HSV + three tables +
 * HSV2BGR, BGR -> RGB.
 *   samples [B]   HOST table (validated before anything touches the device); samples_dev: DEVICE copy of the same table, read by the kernel
 *   minv[l]       invertAffineTransform of layer l's M (layer 0: the sample's mosaic; layer 1: the cached mosaic mixed in)
 *   ntiles[l]     1..MAF_AUGMENT_MAX_TILES tiles for layer 0; 0 (no mixup) or 1..4 for layer 1; r: mixup ratio of layer 0
 *   tile          ptr: DEVICE uint8 HWC frame (pitch bytes, h x w); canvas [x0, x1) x [y0, y1) reads frame pixel (x + dx, y + dy), which
 *                 must lie inside the frame (checked); rectangles of one layer do not overlap
 *   hsv, flipud, fliplr   0 / 1; lut: hue, saturation, value tables (used when hsv = 1)
 *   S             the output side, a positive multiple of 32
 *   out           DEVICE, 4-byte aligned, uint8 [B, 3, S, S]: every byte written exactly once (32-bit stores)
 * maf_augment_sample_size: sizeof(maf_augment_sample_t), for bindings to check their mirror.
 */
#define MAF_AUGMENT_MAX_TILES 4
typedef struct {
    const uint8_t* ptr; int64_t pitch;
    int32_t h, w;                        /* frame */
    int32_t x0, y0, x1, y1;              /* canvas rectangle */
    int32_t dx, dy;                      /* frame pixel = canvas pixel + (dx, dy) */
} maf_augment_tile_t;
typedef struct {
    double minv[2][6];
    double r;
    int32_t ntiles[2];
    int32_t hsv, flipud, fliplr, reserved;
    maf_augment_tile_t tile[2][MAF_AUGMENT_MAX_TILES];
    uint8_t lut[3][256];
} maf_augment_sample_t;
int32_t maf_augment_sample_size(void);
int maf_mosaic_affine(const maf_augment_sample_t* samples, const maf_augment_sample_t* samples_dev, int32_t B, int32_t S, uint8_t* out,
                      maf_stream_t stream);

/*
 * copy_paste on polygon labels (yolov6/data/data_augment.py:285-307), opt-in through TrainAugment(polygons=True) in maf-yolo_amd/augment.py.
 *
 * maf_polygon_mask: for each of n masks, the union of what cv2.drawContours(im_new, [contour], -1, (1, 1, 1), cv2.FILLED) draws for that
 * mask's contours on a C x C canvas, as a bit mask; all masks in one launch.  The fill rule (OpenCV's fillPoly with line_type 8, shift 0:
 * every edge as LineIterator's 8-connected clipped line, plus the even-odd scan-line interior in 16.16 fixed point) is the one restated in
 * tests/copy_paste_ref.py, bit for bit.
 *   table         HOST int32 table (validated before anything touches the device); table_dev: DEVICE copy of the same table (4-byte
 *                 aligned), read by the kernel.  Three arrays back to back:
 *                   mask_start [n + 1]       mask i owns contours [mask_start[i], mask_start[i + 1]); rises from 0 to npoly; a mask may own none
 *                   poly_start [npoly + 1]   contour p owns vertices [poly_start[p], poly_start[p + 1]); rises strictly from 0 to nvert
 *                   xy [2 nvert]             x, y of every vertex, each within [-MAF_POLYGON_COORD_MAX, MAF_POLYGON_COORD_MAX]; vertices may
 *                                            lie outside the canvas, the kernel clips
 *   n, npoly, nvert   1..MAF_POLYGON_MAX_MASKS masks, 0..MAF_POLYGON_MAX_CONTOURS contours, 0..MAF_POLYGON_MAX_VERTICES vertices in all
 *   C             the canvas side, 1..MAF_POLYGON_MAX_CANVAS
 *   masks         DEVICE, 4-byte aligned, uint32 [n, C, W], W = (C + 31) / 32: pixel (x, y) of mask i is bit x & 31 of word
 *                 (i C + y) W + (x >> 5); the padding bits of a row's last word are 0.  Every word is written exactly once (plain stores,
 *                 no memset needed), a mask without contours as zeros.
 */
#define MAF_POLYGON_COORD_MAX 32767
#define MAF_POLYGON_MAX_CANVAS 16384
#define MAF_POLYGON_MAX_MASKS 65535
#define MAF_POLYGON_MAX_CONTOURS (1 << 24)
#define MAF_POLYGON_MAX_VERTICES (1 << 26)
int maf_polygon_mask(const int32_t* table, const int32_t* table_dev, int32_t n, int32_t npoly, int32_t nvert, int32_t C, uint32_t* masks,
                     maf_stream_t stream);

/*
 * maf_mosaic_affine_paste: maf_mosaic_affine with copy_paste's pixels, im[flip(im_new) != 0] = flip(im)[...], applied to the virtual canvas
 * before the warp.  Same samples table, same checks, same output contract (uint8 [B, 3, S, S], every byte written exactly once); a second
 * table gives every sample its masks:
 *   paste [B]     HOST table (validated before anything touches the device); paste_dev: DEVICE copy of the same table, read by the kernel
 *   mask[l]       layer l's mask in maf_polygon_mask's layout for canvas side C (DEVICE, 4-byte aligned), or NULL: nothing pasted in that
 *                 layer.  A mask needs its layer (ntiles[l] > 0) and tile rectangles inside [0, C]^2.
 *   C             the canvas side; must be 2 S
 * Each of warpAffine's four taps at canvas (x, y) inside [0, C)^2 reads canvas (C-1-x, y) when bit (C-1-x, y) of the layer's mask is set,
 * else canvas (x, y); outside [0, C)^2 it reads 114.  A table without any mask gives maf_mosaic_affine's bytes.
 * maf_augment_paste_size: sizeof(maf_augment_paste_t), for bindings to check their mirror.
 */
typedef struct {
    const uint32_t* mask[2];
    int32_t C, reserved;
} maf_augment_paste_t;
int32_t maf_augment_paste_size(void);
int maf_mosaic_affine_paste(const maf_augment_sample_t* samples, const maf_augment_sample_t* samples_dev, const maf_augment_paste_t* paste,
                            const maf_augment_paste_t* paste_dev, int32_t B, int32_t S, uint8_t* out, maf_stream_t stream);

/*
 * maf_resize_area: load_image's cv2.resize INTER_AREA of an evaluation frame larger than the load size (yolov6/data/datasets.py:277-300 with
 * r < 1 and augment off), n frames in one launch, uint8 HWC in, uint8 HWC out.  Both axes shrink or stay (new_w <= w, new_h <= h); the pixel
 * rule is OpenCV's as restated in tests/area_ref.py, bit for bit.  The caller (maf-yolo_amd/letterbox.py) picks the path of every frame with
 * OpenCV's own test and builds the decimation tables in double; the device only multiplies, adds and rounds.
 *   frames [n]    HOST table (validated); frames_dev: DEVICE copy of the same table, read by the kernel (always required)
 *   src           DEVICE, uint8 HWC (3 channels, pixel stride 3, row pitch src_pitch >= 3 w bytes, any alignment); reads stay in
 *                 [row * pitch, + 3 w) of rows < h
 *   dst           DEVICE, uint8 HWC new_h x new_w, pitch 3 new_w, no alignment needed; every byte written once; must not overlap any src
 *   path          MAF_AREA_FAST2: the 2 x 2 average (a + b + c + d + 2) >> 2, iscale_x = iscale_y = 2;  MAF_AREA_FASTN: the integer sum of
 *                 the iscale_y x iscale_x block times inv_area = 1.0f / (iscale_x iscale_y) in fp32, rounded half to even (1 x 1: a copy);
 *                 both need w = iscale_x new_w and h = iscale_y new_h.  MAF_AREA_GENERAL: the tables below.
 *   tables        HOST copy of the table words (int32), tables_dev its DEVICE copy, table_words their count; may be NULL / 0 when no frame
 *                 takes the general path.  Per axis of a general-path frame, at word offsets from the start of the tables: x_start / y_start
 *                 -> start [n_dst + 1] (entry range of every destination index, rising from 0), x_pairs / y_pairs (even) -> the entries,
 *                 two words each: source index, fp32 alpha.  Frames of one size share their tables.
 * Validates everything above on the host copies — every table offset and every source index of every table included — before touching the
 * device.  maf_area_struct_sizes: sizeof(maf_area_frame_t), for bindings to check their mirror.
 */
#define MAF_AREA_FAST2 0
#define MAF_AREA_FASTN 1
#define MAF_AREA_GENERAL 2
typedef struct {
    const uint8_t* src; int64_t src_pitch;
    int32_t h, w;                        /* source frame */
    uint8_t* dst;
    int32_t new_h, new_w;                /* shrunk frame, pitch 3 new_w */
    int32_t path;                        /* MAF_AREA_* */
    int32_t iscale_x, iscale_y;          /* the fast paths' integer factors */
    float inv_area;                      /* 1.0f / (iscale_x iscale_y) */
    int32_t x_start, x_pairs;            /* the general path's tables, word offsets */
    int32_t y_start, y_pairs;
} maf_area_frame_t;
int maf_area_struct_sizes(int32_t* frame_size);
int maf_resize_area(const maf_area_frame_t* frames, const maf_area_frame_t* frames_dev, int32_t n, const void* tables, const void* tables_dev,
                    int64_t table_words, maf_stream_t stream);

/*
 * In-process precision / recall / mAP of an evaluation (the do_pr_metric path of Evaler.predict_model, yolov6/core/evaler.py:195-268, with
 * yolov6/utils/metrics.py process_batch, ConfusionMatrix, ap_per_class, compute_ap); the rules are those of tests/pr_metric_ref.py.
 * Every pointer below is a DEVICE pointer; nothing synchronises the host.
 *
 * state [maf_pr_state_ints(nc)] int32, zeroed by the caller before the first batch: [0] error bits (MAF_PR_ERR_*), [1] 1 once any row
 *   is correct at any threshold, [2, 2 + nc) labels per class, [2 + nc, 2 + 2 nc) predictions per class, then the confusion matrix
 *   [nc + 1][nc + 1] (row: detected class, column: true class; index nc = background).
 *
 * maf_pr_match: one batch, one workgroup per image.
 *   rows [B][max_det][6] fp32, count [B] int32   the maf_nms result (letterboxed xyxy, conf, cls); max_det <= MAF_PR_MAX_DET
 *   targets [n_targets][6] fp32                  image index in the batch, class, x, y, w, h normalised to the letterboxed H x W, in any
 *                                                image order (order within an image is kept); flags & MAF_PR_LABELS_XYXY: class, x1, y1,
 *                                                x2, y2 in native pixels and no rescale of labels or detections (img_params unused)
 *   img_params [B][6] fp32                       maf_coco_rows' image parameters (h0, w0, gain x, gain y, pad w, pad h)
 *   iouv [niou] fp32, niou <= 16                 thresholds, compared with >=
 *   flags & MAF_PR_CONFUSION                     update the confusion matrix (detections with conf > cm_conf, iou > cm_iou, fp32)
 *   offs_in [1] int64                            record index of this batch's first detection; offs_out [1] := offs_in + rows of the batch
 *   keys, masks [capacity]                       per detection (at offs_in + rows of earlier images + row): key = class << 32 | the
 *                                                descending-order bits of conf; mask bit t = correct at iouv[t].  Slots never written keep
 *                                                the caller's fill (INT64_MAX for keys).
 *   Device-side errors (a class outside [0, nc) or not integral, more than MAF_PR_MAX_LABELS labels in an image, records past capacity)
 *   set bits of state[0]; the launch itself succeeds.
 *
 * maf_pr_curves: once per evaluation, on the keys sorted ascending by a STABLE sort (sorted_keys, perm = the sort's indices into keys /
 *   masks): per-class offsets, then one workgroup per (class, threshold), then the summary.  workspace: maf_pr_workspace_bytes(nc, niou,
 *   capacity) bytes.  out [maf_pr_out_doubles(nc, niou)] fp64: header [MAF_PR_HEADER] (F1 index, mp, mr, mf1, map50, map, classes with
 *   labels, any correct, error bits), then p, r, f1, py [nc][1000], ap [nc][niou], labels per class [nc], confusion [(nc+1)^2].  Rows of
 *   classes without labels are not summarised (callers keep the rows with labels > 0: np.unique of the target classes).
 */
#define MAF_PR_MAX_DET 1024
#define MAF_PR_MAX_LABELS 1024
#define MAF_PR_MAX_CLASSES 1024
#define MAF_PR_HEADER 16
#define MAF_PR_LABELS_XYXY 1
#define MAF_PR_CONFUSION 2
#define MAF_PR_ERR_CLASS 1
#define MAF_PR_ERR_LABELS 2
#define MAF_PR_ERR_CAPACITY 4
int64_t maf_pr_state_ints(int32_t nc);
int64_t maf_pr_out_doubles(int32_t nc, int32_t niou);
int64_t maf_pr_workspace_bytes(int32_t nc, int32_t niou, int64_t capacity);
int maf_pr_match(const float* rows, const int32_t* count, int32_t B, int32_t max_det, const float* targets, int32_t n_targets,
                 const float* img_params, int32_t H, int32_t W, const float* iouv, int32_t niou, int32_t nc, int32_t flags,
                 float cm_conf, float cm_iou, const int64_t* offs_in, int64_t* offs_out, int64_t* keys, uint16_t* masks,
                 int64_t capacity, int32_t* state, maf_stream_t stream);
int maf_pr_curves(const int64_t* sorted_keys, const int64_t* perm, const uint16_t* masks, int64_t capacity, const int32_t* state,
                  int32_t nc, int32_t niou, void* workspace, int64_t workspace_bytes, double* out, maf_stream_t stream);

/*
 * COCO bbox mAP (pycocotools' COCOeval, iouType 'bbox', useCats 1, as Evaler.eval_model runs it, yolov6/core/evaler.py:276-364); the rules
 * are those of tests/cocoeval_ref.py.  Every pointer below is a DEVICE pointer; nothing synchronises the host.  T = 10 IoU thresholds,
 * R = 101 recall thresholds, A = 4 area ranges, M = 3 maxDets (MAF_COCO_*); the parameters travel as the host's doubles.
 *
 * maf_coco_append: one batch of maf_coco_rows output -> detection records.  packed [rows][7] fp32 (batch image, category id, x, y, w, h,
 *   score), total [1] int32 (rows past it are written as padding); img_index [B] int32: batch image -> gt image index; cat_lut [n_lut] int32:
 *   category id -> category index or -1.  Per row: det_img / det_cat int32 (-1: padding / unknown category), det_box [4] fp64 =
 *   rint(v * 1000) / 1000, det_score fp64 = rint(v * 1e5) / 1e5.
 *
 * maf_coco_match: one workgroup per (image, category) cell c = image * K + category.  The gt records are sorted by cell (JSON order within),
 *   gt_off [I * K + 1]; gt_flags: MAF_COCO_GT_CROWD | MAF_COCO_GT_IDNZ (the annotation id is nonzero); at most MAF_COCO_MAX_GT per cell.
 *   cell_keys [n] ascending (stable sort of the records by cell after a stable sort by score descending; INT64_MAX: not evaluated), order [n]:
 *   the record index of each sorted position.  img_sel [I] uint8, cat_map [K] int32 (>= 0: evaluated).  iou_thrs [T], area_rng [A][2] fp64.
 *   Per sorted position of the first MAF_COCO_MAX_DETS of a cell: rank (the caller fills -1 first), mbits / ibits (bit a * T + t: matched to
 *   a gt with a nonzero id / ignored); npig [I * K][A] int32: non-ignored gts per cell and area range.
 *
 * maf_coco_accumulate: cat_keys [n] ascending (the evaluated category index k' of each kept position, INT64_MAX otherwise; stable sort after a
 *   stable sort by score descending of the cell-ordered positions) with rank / mbits / ibits / score gathered in that order.  cat_of [Kp]:
 *   k' -> category index (-1: no such category).  rec_thrs [R] fp64, max_dets [M] int32.  precision, scores [T][R][Kp][A][M] and recall
 *   [T][Kp][A][M] fp64 are written whole (-1 where pycocotools leaves -1).
 */
#define MAF_COCO_T 10
#define MAF_COCO_R 101
#define MAF_COCO_A 4
#define MAF_COCO_M 3
#define MAF_COCO_MAX_DETS 100
#define MAF_COCO_MAX_GT 256
#define MAF_COCO_GT_CROWD 1
#define MAF_COCO_GT_IDNZ 2
int maf_coco_append(const float* packed, const int32_t* total, int64_t rows, const int32_t* img_index, int32_t B, const int32_t* cat_lut,
                    int32_t n_lut, int32_t* det_img, int32_t* det_cat, double* det_box, double* det_score, maf_stream_t stream);
int maf_coco_match(const double* gt_box, const double* gt_area, const uint8_t* gt_flags, const int64_t* gt_off, const int64_t* cell_keys,
                   const int64_t* order, const double* det_box, int64_t n, const uint8_t* img_sel, const int32_t* cat_map, int32_t I, int32_t K,
                   const double* iou_thrs, const double* area_rng, int32_t* rank, uint64_t* mbits, uint64_t* ibits, int32_t* npig,
                   maf_stream_t stream);
int maf_coco_accumulate(const int64_t* cat_keys, const int32_t* rank, const uint64_t* mbits, const uint64_t* ibits, const double* score, int64_t n,
                        const int32_t* npig, const uint8_t* img_sel, const int32_t* cat_of, int32_t I, int32_t K, int32_t Kp,
                        const double* rec_thrs, const int32_t* max_dets, double* precision, double* recall, double* scores, maf_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------------------------
 * Baseline JPEG decoding on the device (csrc/jpeg_decode.hip): what cv2.imread (libjpeg with its defaults: JDCT_ISLOW, fancy upsampling,
 * BGR) returns for a file, bit for bit; the rules are those of tests/jpeg_ref.py.  SOF0, 8 bit, Huffman, one interleaved scan, 1 or 3
 * components (Y 1x1, 2x1 or 2x2 with 1x1 chroma).  The host walks the markers (maf-yolo_amd/jpeg.py) and hands over ONE byte blob, copied
 * to the device as it is: maf_jpeg_header_t | maf_jpeg_image_t [n_images] | maf_jpeg_lane_t [n_lanes] | Huffman table sets | quantisation
 * tables (uint16 [3][64] per image, natural order) | the scans' bytes followed by at least MAF_JPEG_SCAN_PAD zero bytes.
 *
 * Stages of a call (one chain of launches on `stream`, nothing synchronises; `stages` selects them, MAF_JPEG_STAGE_ALL for a decode):
 *   ENTROPY  jdhuff.c decode_mcu: one lane per restart interval (per image without DRI), `group` lanes per one-wave workgroup sharing one
 *            Huffman table set in LDS; 0xFF00 unstuffed on the fly; DC prediction reset per lane and component; int16 coefficients in
 *            natural order (jutils.c jpeg_natural_order) for every block of every MCU (jdcoefct.c), component after component, blocks
 *            row-major over the component padded to whole MCUs.  The reader's byte index is clamped into the scan buffer, so no stream
 *            content reads or writes outside the buffers; faults set bits of status[image] (MAF_JPEG_ST_*) instead.
 *   IDCT     jidctint.c jpeg_idct_islow with dequantisation and the range-limit table of jdmaster.c -> uint8 component planes padded to
 *            whole MCUs (pitch 8 * blocks per row).
 *   COLOR    jdsample.c h2v1_fancy_upsample / h2v2_fancy_upsample (the box replication of h2v1_upsample / h2v2_upsample where the chroma
 *            plane is at most 2 samples wide), the edge rules of jdmainct.c, jdcolor.c ycc_rgb_convert's 16-bit tables -> uint8 [h][w][3]
 *            BGR at out + out_off; a one-component file writes its gray value three times.  An image whose `orientation` is 2 to 8 is
 *            written through that EXIF orientation instead: the stored pixel (x, y) goes to (x', y') of a frame of w x h (2 to 4) or h x w
 *            (5 to 8) pixels, x' = x or w - 1 - x (orientations 2, 3, 7, 8), y' = y or h - 1 - y (3, 4, 6, 7), the two exchanged for 5 to
 *            8; the same 3 * w * h bytes at out + out_off (rules restated in tests/jpeg_orientation_ref.py).
 *
 * A Huffman table set is 4 tables (DC 0, DC 1, AC 0, AC 1) of MAF_JPEG_HUFF_TABLE_BYTES: look uint16 [512] (length << 8 | symbol for every
 * 9-bit prefix that starts with a code of at most 9 bits, else 0), maxcode int32 [18] (-1: no code of that length), valoff int32 [18]
 * (symbol = huffval[valoff[l] + code]), huffval uint8 [256].  Lanes [group g, group (g + 1)) share one tabset; padding lanes have image -1.
 * maf_jpeg_decode validates the whole HOST copy of the blob (every offset, size and index) before it touches the device.
 *
 * Progressive files (SOF2; csrc/jpeg_progressive.hip, rules restated in tests/jpeg_progressive_ref.py) ride in the same blob when the header's
 * n_scans > 0: behind the quantisation tables follow maf_jpeg_scan_t [n_scans] | maf_jpeg_lane_t [n_slanes] (the "scan lanes") | int32
 * [n_rounds + 1] round starts.  A progressive image has a maf_jpeg_image_t like any other (its dc_tab / ac_tab unused) and no lane in the
 * baseline lane table; every scan of it has one row in the scan table (rows sorted by image, then by `round` = the scan's position in its
 * file) and one scan lane per restart interval OF THAT SCAN, whose `image` field holds the scan-table row and whose first_mcu / n_mcu count
 * the scan's own MCUs: the frame's MCUs in the interleaved DC scan of all components, single blocks of a bw x bh grid over the component's
 * own ceil(samples / 8) in a one-component scan (jdinput.c per_scan_setup), addressed inside the padded coefficient planes above.
 * Scan lanes [rounds[k], rounds[k + 1]) belong to round k: the k-th scan of every image that has one.  The ENTROPY stage launches
 * jpeg_entropy_kernel over the baseline lanes (if any) and then jpeg_prog_entropy_kernel once per round, in order on the stream: at most
 * max-scans-per-image launches whatever the batch.  It restates jdphuff.c decode_mcu_DC_first / DC_refine / AC_first / AC_refine; the one
 * lane that owns a block in a scan reads, modifies and writes its coefficients with ordinary loads and stores.  EOBRUN is lane state, zero at
 * every restart.  Scan lanes come in groups of `sgroup` sharing one table set, as the baseline lanes do in groups of `group`.
 */
#define MAF_JPEG_GROUP 64
#define MAF_JPEG_SCAN_PAD 64
#define MAF_JPEG_HUFF_TABLE_BYTES 1424
#define MAF_JPEG_ST_BAD_CODE 1      /* no Huffman code matches, or a DC category above 16 */
#define MAF_JPEG_ST_BAD_INDEX 2     /* an AC run moves past coefficient 63 */
#define MAF_JPEG_ST_SHORT_SCAN 4    /* the interval's bytes ran out before its MCUs did */
#define MAF_JPEG_ST_REFINE_PAST_SE 8 /* progressive: an AC run (first pass or refinement) places a coefficient past the scan's Se */
#define MAF_JPEG_STAGE_ENTROPY 1
#define MAF_JPEG_STAGE_IDCT 2
#define MAF_JPEG_STAGE_COLOR 4
#define MAF_JPEG_STAGE_ALL 7
typedef struct {
    int32_t n_images, n_lanes, n_tabsets;    /* n_lanes: the baseline lanes (0 where every file is progressive) */
    int32_t group;                           /* decoding lanes per workgroup, 1 to MAF_JPEG_GROUP; n_lanes is a multiple of it */
    int64_t images_off, lanes_off, huff_off, quant_off, scan_off;   /* byte offsets of the sections in the blob (16-byte aligned) */
    int64_t scan_bytes;                      /* the scans' bytes including the zero padding */
    int64_t total_bytes;                     /* of the blob */
    int64_t coef_elems, plane_bytes, out_bytes;   /* sizes of the three device buffers */
    int32_t n_scans, n_slanes, n_rounds;     /* progressive: scan-table rows, scan lanes, rounds; all 0 in a call without progressive files */
    int32_t sgroup;                          /* scan lanes per workgroup, 1 to MAF_JPEG_GROUP; every round's lane count is a multiple of it */
    int64_t scans_off, slanes_off, rounds_off;
} maf_jpeg_header_t;
typedef struct {
    int64_t coef_off;                        /* int16 elements, a multiple of 64 */
    int64_t plane_off;                       /* bytes, a multiple of 64 */
    int64_t out_off;                         /* bytes, a multiple of 16 */
    int32_t w, h, ncomp;                     /* ncomp 1 or 3 */
    int32_t hs, vs;                          /* luma sampling factors (1,1), (2,1) or (2,2); chroma is 1 x 1 */
    int32_t mcux, mcuy;                      /* ceil(w / (8 hs)), ceil(h / (8 vs)) */
    int32_t quant;                           /* index of the image's first quantisation table */
    int32_t dc_tab[3], ac_tab[3];            /* per component: table 0 or 1 of the set */
    int32_t orientation;                     /* 0 or 1: the stored grid; 2 to 8: the frame is written through that EXIF orientation (for 5 to 8 it is [w][h][3]) */
    int32_t reserved;
} maf_jpeg_image_t;
typedef struct {
    int64_t begin, end;                      /* byte range of the interval inside the scan buffer (markers excluded) */
    int32_t image;                           /* -1: a padding lane */
    int32_t first_mcu, n_mcu;
    int32_t tabset;
} maf_jpeg_lane_t;
typedef struct {
    int32_t image;
    int32_t round;                           /* the scan's position among its image's scans = the launch it is decoded in */
    int32_t ncomp;                           /* components in the scan: the image's ncomp (interleaved DC scan) or 1 */
    int32_t comp[3];                         /* their indices in frame order: 0, 1, 2 when interleaved, else comp[0] */
    int32_t ss, se, ah, al;                  /* ss == 0 implies se == 0; otherwise ncomp == 1 and ss <= se <= 63; al <= 13; ah == 0 or al + 1 */
    int32_t dc_tab[3];                       /* DC scans: table 0 or 1 of the lane's set, per scan component */
    int32_t ac_tab;                          /* AC scans: table 0 or 1 */
    int32_t bw, bh;                          /* the scan's MCU grid (see above) */
} maf_jpeg_scan_t;
int maf_jpeg_struct_sizes(int32_t* header_image_lane);   /* sizeof of the three structs above (binding check) */
int maf_jpeg_progressive_struct_sizes(int32_t* scan);    /* sizeof(maf_jpeg_scan_t) */
int maf_jpeg_decode(const void* blob_host, const void* blob_dev, int16_t* coef, uint8_t* planes, uint8_t* out, int32_t* status,
                    int32_t stages, maf_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------------------------
 * Baseline JPEG encoding on the device (csrc/jpeg_encode.hip): uint8 BGR frames, or rectangles of them, in; the files libjpeg writes with
 * its defaults out (jpeg_set_quality with force_baseline, JDCT_ISLOW, 4:2:0 or 4:4:4, the standard Huffman tables, JFIF header), bit for bit;
 * the rules are those of tests/jpeg_encode_ref.py.  The host (maf-yolo_amd/jpeg_encode.py) hands over ONE byte blob, copied to the device as
 * it is: maf_jpeg_enc_header_t | maf_jpeg_enc_job_t [n_files] | Huffman code tables: uint32 [4][256] (DC luma, DC chroma, AC luma, AC
 * chroma; length << 16 | code for a symbol, 0 where it has none) | divisors: uint16 [2][64] (luma, chroma; natural order, the quantisation
 * value, not yet times 8) | the files' headers (everything in front of the scan), byte after byte.
 *
 * One chain of launches on `stream` for the whole batch, whatever the number of files; nothing synchronises:
 *   transform  one thread per 8 x 8 block of the batch, blocks in the order they are coded (MCUs in raster order; Y blocks, Cb, Cr): colour
 *              conversion straight from the strided frame (jccolor.c), edge padding by index clamping, h2v2 downsampling (jcsample.c), the
 *              islow FDCT (jfdctint.c), quantisation (jcdctmgr.c) -> int16 [64] per block in zigzag order.
 *   count      bits per block (jchuff.c) with the DC difference against the nearest coded real block of the same component; a dummy block
 *              (jccoefct.c) receives that block's DC and costs the fixed DC-category-0 + EOB; sums per 256 blocks.
 *   offsets    exclusive scan of the bit counts over all blocks of the batch (two levels; 64-bit) -> bitoff [n_blocks + 1].
 *   pack       every block writes its codes at its bit offset inside its file's region of `packed` (zeroed on the stream by this call;
 *              words two blocks share are combined with atomicOr); the last block fills the final byte with 1-bits.
 *   stuff      0xFF bytes counted per MAF_JPEG_ENC_CHUNK packed bytes, scanned per file, file lengths scanned over the batch; then header,
 *              stuffed scan and EOI of every file are written back to back into `out`: file i at offsets[i], lengths[i] bytes long.
 * Worst case per block, by which the host sizes `packed` and `out`: MAF_JPEG_ENC_BLOCK_BITS = 22 (the longest DC code, 11 bits for
 * category 11 of the chroma table, + 11 value bits) + 63 x 26 (a 16-bit AC code + 10 value bits for every coefficient) = 1 660 bits, 208
 * bytes; twice that once stuffed.  The kernels hold every block to it (sizes are clamped to 11 and 10) whatever the pixels are.
 * maf_jpeg_encode validates the whole HOST copy of the blob before it touches the device.  It cannot see the frames' allocations: that
 * `src` + rows x pitch lies inside one is the caller's to check.
 */
#define MAF_JPEG_ENC_BLOCK_BITS 1660
#define MAF_JPEG_ENC_BLOCK_BYTES 208   /* ceil(MAF_JPEG_ENC_BLOCK_BITS / 8) */
#define MAF_JPEG_ENC_CHUNK 4096        /* bytes of `packed` one workgroup of the stuffing kernels covers; a file's region is whole chunks */
#define MAF_JPEG_ENC_MAX_BLOCKS (1 << 20)   /* blocks per file: keeps a file's bit offsets inside 31 bits */
typedef struct {
    int32_t n_files;
    int32_t n_blocks;                        /* of the whole batch */
    int32_t n_chunks;                        /* of the whole batch: `packed` holds n_chunks * MAF_JPEG_ENC_CHUNK bytes */
    int32_t reserved;
    int64_t jobs_off, huff_off, quant_off, heads_off;   /* byte offsets of the sections in the blob (16-byte aligned) */
    int64_t heads_bytes;
    int64_t total_bytes;                     /* of the blob */
    int64_t out_bytes;                       /* capacity of `out`: at least the sum over the files of head_len + 2 + 2 * MAF_JPEG_ENC_BLOCK_BYTES * n_blocks */
} maf_jpeg_enc_header_t;
typedef struct {
    const void* src;                         /* device pointer to the first pixel of the frame or rectangle: uint8, pixel stride 3 (B, G, R) */
    int64_t pitch;                           /* bytes between rows, at least 3 * w */
    int32_t w, h;                            /* 1 to 65535 */
    int32_t hs;                              /* luma sampling factor in both directions: 2 (4:2:0) or 1 (4:4:4) */
    int32_t mcux, mcuy;                      /* ceil(w / (8 hs)), ceil(h / (8 hs)) */
    int32_t block0, n_blocks;                /* the file's blocks in the batch: n_blocks = mcux * mcuy * (hs * hs + 2) */
    int32_t chunk0, n_chunks;                /* its region of `packed`: n_chunks = ceil(n_blocks * MAF_JPEG_ENC_BLOCK_BYTES / MAF_JPEG_ENC_CHUNK) */
    int32_t head_off, head_len;              /* its header inside the heads section */
    int32_t reserved;
} maf_jpeg_enc_job_t;
int maf_jpeg_encode_struct_sizes(int32_t* header_job);   /* sizeof of the two structs above (binding check) */
/* coef int16 [64 * n_blocks], bits int32 [n_blocks], bitoff int64 [n_blocks + 1], sums int64 [2 * ceil(n_blocks / 256)], packed uint8
 * [n_chunks * MAF_JPEG_ENC_CHUNK], ffcount int32 [n_chunks], out uint8 [out_bytes], lengths int32 [n_files], offsets int64 [n_files]; all
 * device buffers, blob_dev / coef / packed 16-byte aligned. */
int maf_jpeg_encode(const void* blob_host, const void* blob_dev, int16_t* coef, int32_t* bits, int64_t* bitoff, int64_t* sums, uint8_t* packed,
                    int32_t* ffcount, uint8_t* out, int32_t* lengths, int64_t* offsets, maf_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------------------------
 * PNG decoding on the device (csrc/png_decode.hip): what cv2.imread (IMREAD_COLOR: libpng with png_set_strip_16, png_set_strip_alpha,
 * png_set_palette_to_rgb, png_set_expand_gray_1_2_4_to_8, png_set_gray_to_rgb, png_set_bgr) returns for a non-interlaced or an Adam7 file,
 * bit for bit; the rules are those of tests/png_ref.py and tests/png_adam7_ref.py.  The host walks the chunks (maf-yolo_amd/png.py: CRC-32 of the critical chunks, IHDR,
 * PLTE, the zlib header) and hands over ONE byte blob, copied to the device as it is: maf_png_header_t | maf_png_image_t [n_images] |
 * palette entries uint8 [n_palette][4] (B, G, R, 0) | the zlib streams of every image (its IDAT payloads concatenated, chunk framing
 * removed) followed by at least MAF_PNG_STREAM_PAD zero bytes.
 *
 * Stages of a call (one chain of launches on `stream`, nothing synchronises; `stages` selects them, MAF_PNG_STAGE_ALL for a decode):
 *   INFLATE   RFC 1951, one one-wave workgroup per image, every lane decoding the same symbol (no divergence) and the 64 lanes moving the
 *             bytes of a literal run, a stored block or a match together -> the filtered scanlines, exactly h * (1 + rowbytes) bytes at
 *             inflated + inf_off.  The Adler-32 is not verified.
 *   UNFILTER  PNG filter types 0 to 4 undone, lane k of a wave on row y0 + k one pixel behind lane k - 1 -> uint8 [h][rowbytes] at rows +
 *             rows_off.
 *   CONVERT   the conversion table of maf-yolo_amd/png.py -> uint8 [h][w][3] BGR at out + out_off.
 * An image with interlace = 1 (Adam7; PNG 1.2, 8.2) rides in the same launches.  Pass p = 0 .. 6 holds the pixels (x0 + i dx, y0 + j dy),
 * (x0, y0, dx, dy) = (0,0,8,8) (4,0,8,8) (0,4,4,8) (2,0,4,4) (0,2,2,4) (1,0,2,2) (0,1,1,2), as a sub-image of pw = ceil((w - x0) / dx) by
 * ph = ceil((h - y0) / dy) pixels with rows of prb = ceil(pw * channels * depth / 8) bytes; a pass with pw or ph 0 is absent.  INFLATE
 * produces the sum of ph * (1 + prb) bytes; UNFILTER (a grid of images x 7 when the call holds such an image) undoes every pass as a filter
 * chain of its own, its first row with zeros above it, and writes the sub-images back to back at rows + rows_off, the sum of ph * prb bytes
 * (for depths below 8 that can exceed h * rowbytes); CONVERT gathers pixel (x, y) from the pass that (x & 7, y & 7) names.  The kernels derive
 * the geometry from w, h, depth and ctype; the blob has no section for it.
 * Bounded by construction: every input byte index is clamped into the stream section and compared with the image's stream_end, past which
 * the reader feeds zeros; every output index is compared with inflated_size; every distance with the bytes produced so far; every loop has
 * a bound the host validated or a constant one.  A malformed stream ends with bits of status[image] (MAF_PNG_ST_*) and a zero-filled
 * remainder.  maf_png_decode validates the whole HOST copy of the blob (every offset, size, count and index) before it touches the device.
 */
#define MAF_PNG_STREAM_PAD 64
#define MAF_PNG_ST_INPUT_EXHAUSTED 1    /* bits past the end of the image's stream were consumed */
#define MAF_PNG_ST_BAD_BLOCK_TYPE 2     /* BTYPE 3 */
#define MAF_PNG_ST_BAD_STORED_LEN 4     /* a stored block whose LEN is not ~NLEN */
#define MAF_PNG_ST_BAD_CODE_LENGTHS 8   /* an over-subscribed or incomplete code, more than 286 / 30 symbols, a repeat with nothing to repeat or past the end, no end-of-block code */
#define MAF_PNG_ST_NO_CODE 16           /* no code matches the bits, or a length symbol above 285 / a distance symbol above 29 */
#define MAF_PNG_ST_DISTANCE_TOO_FAR 32  /* a distance larger than the bytes produced so far */
#define MAF_PNG_ST_TOO_MANY_BYTES 64    /* the stream holds more than inflated_size bytes */
#define MAF_PNG_ST_TOO_FEW_BYTES 128    /* the stream ends before inflated_size bytes */
#define MAF_PNG_ST_BAD_FILTER 256       /* a filter type above 4 (the row is taken as type 0) */
#define MAF_PNG_ST_BAD_PALETTE_INDEX 512 /* a palette index past PLTE (the pixel is black) */
#define MAF_PNG_STAGE_INFLATE 1
#define MAF_PNG_STAGE_UNFILTER 2
#define MAF_PNG_STAGE_CONVERT 4
#define MAF_PNG_STAGE_ALL 7
typedef struct {
    int32_t n_images, n_palette;             /* n_palette: palette entries of the whole call */
    int64_t images_off, palette_off, stream_off;   /* byte offsets of the sections in the blob (16-byte aligned) */
    int64_t stream_bytes;                    /* the streams' bytes including the zero padding, a multiple of 8 */
    int64_t total_bytes;                     /* of the blob */
    int64_t inflated_bytes, rows_bytes, out_bytes;   /* sizes of the three device buffers */
} maf_png_header_t;
typedef struct {
    int64_t stream_begin, stream_end;        /* the image's deflate bytes inside the stream section: the 2-byte zlib header excluded, the Adler-32 included */
    int64_t inf_off, rows_off, out_off;      /* bytes, multiples of 16 */
    int32_t w, h;                            /* 1 to 65535 */
    int32_t depth, ctype;                    /* IHDR: 1 / 2 / 4 / 8 / 16 and 0 gray, 2 RGB, 3 palette, 4 gray + alpha, 6 RGBA */
    int32_t rowbytes;                        /* ceil(w * channels * depth / 8) */
    int32_t bpp;                             /* the filters' byte distance: max(1, channels * depth / 8) */
    int32_t inflated_size;                   /* h * (1 + rowbytes), Adam7: the sum of ph * (1 + prb) over the non-empty passes; below 2^31 */
    int32_t pal, pal_n;                      /* ctype 3: first palette entry and their number (1 to 256) */
    int32_t interlace;                       /* IHDR's interlace method: 0 none, 1 Adam7 (anything else is refused) */
} maf_png_image_t;
int maf_png_struct_sizes(int32_t* header_image);   /* sizeof of the two structs above (binding check) */
/* inflated uint8 [inflated_bytes], rows uint8 [rows_bytes], out uint8 [out_bytes], status int32 [n_images]: device buffers, the first three
 * and blob_dev 16-byte aligned.  status is cleared by the INFLATE stage only; UNFILTER and CONVERT OR their bits into what it holds, and each
 * stage reads what the stage before it wrote.  A mask without MAF_PNG_STAGE_INFLATE is therefore for measuring a stage on buffers that a full
 * decode has filled (tools/png_probe.py); a decode passes MAF_PNG_STAGE_ALL. */
int maf_png_decode(const void* blob_host, const void* blob_dev, uint8_t* inflated, uint8_t* rows, uint8_t* out, int32_t* status,
                   int32_t stages, maf_stream_t stream);

/* Diagnostics: shader-clock cycle stamps of image 0 of the last maf_nms call (synchronises the device):
 * [0] sort, [1] kept-list screening, [2] wave resolution, [3] total, [4] candidates, [5] survivors. */
int maf_nms_debug(uint64_t* host8);

/* HIP-event timing helper used by bench.py (events recorded on `stream`, not torch's). */
int maf_timer_create(void** timer);
int maf_timer_start(void* timer, maf_stream_t stream);
int maf_timer_stop(void* timer, maf_stream_t stream);
int maf_timer_elapsed_ms(void* timer, float* ms);   /* synchronises on the stop event */
void maf_timer_destroy(void* timer);

#ifdef __cplusplus
}
#endif
#endif
