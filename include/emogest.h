/*
 * emogest.h -- C ABI of libemogest_hip.so: the MI355X (gfx950) implementation of the
 * EmotionGesture audio->gesture hot path.
 *
 * The reference (XingqunQi-lab/EmotionGestures) is pure Python/PyTorch and has no FFI; the
 * boundary it exposes for this path is the nn.Module surface used by
 * test_emotion_gesture_diversity_iterative.py:25-30,135-174,203-205.  Each entry point below
 * names the reference function it replaces (paths relative to the upstream repo).  The Python
 * host mirror (emotiongestures_amd.Full_model.*, emotiongestures_amd.CAVE.*) binds these with
 * ctypes; INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Contract (all entry points):
 *   - plain C types only; every pointer named "d_*"/"arena"/"workspace" or documented as
 *     device memory is a HIP device pointer owned by the CALLER (PyTorch's caching allocator
 *     in the host mirror).  The library never allocates, frees or copies device memory behind
 *     the caller's back and never synchronises the device.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing touches
 *     the default stream.
 *   - return value: EG_OK (0) or a negative EgStatus; HIP launch errors are surfaced as
 *     EG_ERR_HIP.  No exceptions cross the ABI.  eg_last_error() gives a thread-local message.
 *   - stateless and re-entrant: EgGenerator / EgCvae handles are immutable host-side plans
 *     (offset tables); they hold no device memory and may be shared by threads.
 *   - activations are fp32 in HBM.  Convolution activations are NHWC inside the library; every
 *     tensor crossing this ABI uses the reference's own layout (stated per function).
 */
#ifndef EMOGEST_H
#define EMOGEST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum EgStatus {
    EG_OK = 0,
    EG_ERR_BAD_ARG = -1,        /* null pointer, negative size, inconsistent shape */
    EG_ERR_UNSUPPORTED = -2,    /* shape / channel count the kernels are not built for */
    EG_ERR_WORKSPACE = -3,      /* workspace too small (see *_workspace_bytes) */
    EG_ERR_HIP = -4,            /* hipGetLastError() != hipSuccess after a launch */
    EG_ERR_ALIGN = -5           /* pointer or leading dimension not 16-byte aligned */
} EgStatus;

/* Arithmetic mode of the contraction kernels (conv / GEMM).  Storage is fp32 in both. */
typedef enum EgPrecision {
    EG_PREC_F32 = 0,            /* v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulate */
    EG_PREC_BF16X3 = 1,         /* split-bf16: hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 */
    EG_PREC_BF16 = 2            /* single bf16 product (fast mode; not parity-grade) */
} EgPrecision;

const char* eg_last_error(void);
const char* eg_version(void);
/* Process-wide default for the contraction kernels (EgPrecision).  Per-call structs below
 * carry their own field; this only seeds eg_*_default_config. */
int eg_set_default_precision(int precision);
int eg_get_default_precision(void);

/* Number of kernel launches the library has issued in this process (every launch function counts; captured launches count when they are
 * recorded, not when a hipGraph replays them).  bench.py reports launches per step from differences of this counter. */
int64_t eg_launch_count(void);
/* Diagnostic (process started with EG_LAUNCH_HIST=1, else empty): launches by launch-site label since the last reset, as "label count\n" lines
 * written NUL-terminated into buf (truncated to cap); returns the bytes the full text needs.  reset != 0 clears the counts. */
int64_t eg_launch_histogram(char* buf, int64_t cap, int32_t reset);
/* Optional per-launch timing of the contraction kernels (bench.py's roofline leg; a debugging facility, process
 * global, not thread safe).  While enabled, every eg_conv3x3 / eg_linear launch is bracketed by a hipEvent pair on its
 * own stream (no synchronisation).  eg_profile_read synchronises those events and returns, per record, a tag
 * (conv: cin*1000000 + cout*1000 + stride*100 + 1; linear: 2 = LDS-DMA kernel, 3 = pre-split-input kernel, 4 = causal-shift
 * kernel, 5 = f32 kernel), its work in FLOP and its duration in ms. */
int eg_profile_enable(int32_t max_records);
int eg_profile_disable(void);
int32_t eg_profile_read(int64_t* tags, double* flops, float* ms, int32_t capacity);
/* Workgroups of each recorded launch (0: not recorded -- a grid that covers the chip), in record order; call BEFORE eg_profile_read (which
 * resets the record list).  A product on 68 workgroups occupies a quarter of the 256 CUs for its duration: bench.py weighs a launch's
 * duration with min(1, workgroups / 256) when it reports the CU time of a kernel family beside its stand-alone duration. */
int32_t eg_profile_read_workgroups(int32_t* workgroups, int32_t capacity);

/* ------------------------------------------------------------------------------------------
 * Weight arena.  A model's parameters live in ONE caller-owned fp32 device buffer ("arena")
 * in kernel-ready layouts.  The library is authoritative for the layout: it publishes a
 * manifest (one entry per packed tensor) naming the reference state_dict key(s) each entry is
 * built from and the packing rule; the host packs on the CPU once per load_state_dict and
 * uploads.  Offsets and sizes are in floats.
 * ------------------------------------------------------------------------------------------ */
typedef enum EgPackKind {
    EG_PACK_RAW = 0,            /* tensor copied as is (row-major) */
    EG_PACK_LINEAR = 1,         /* nn.Linear weight [N,K] -> fp32 [Npad,Kpad] + tile-planar bf16 hi/lo images; Npad,Kpad % 64 == 0
                                   (dims = N,K,Npad,Kpad; numel = 2*Npad*Kpad floats) */
    EG_PACK_VEC_PAD = 2,        /* 1-D tensor zero padded to dims[1] (dims = n, npad) */
    EG_PACK_CONV3X3 = 3,        /* Conv2d OIHW [O,I,3,3] -> [tap][I/4][Opad][4] (dims = O,I,Opad) */
    EG_PACK_BN_SCALE = 4,       /* key = BN prefix: weight/sqrt(running_var+eps), padded to dims[1] with 0 */
    EG_PACK_BN_SHIFT = 5,       /* key = BN prefix: bias - running_mean*scale, padded to dims[1] with 0 */
    EG_PACK_CONV1X1 = 6,        /* Conv2d [O,I,1,1] -> [I][O] */
    EG_PACK_STEM = 7,           /* Conv2d [O,1,3,3] -> [9][O] */
    EG_PACK_WN_TAP = 8,         /* key = weight-norm conv prefix (weight_g, weight_v [O,I,k]); tap dims[2] of
                                   g*v/||v|| as [O,Ipad] (dims = O,I,tap,Ipad) */
    EG_PACK_CONV1D = 9,         /* Conv1d [O,I,k] -> [O][I][k] raw (alias of RAW, kept for readability) */
    EG_PACK_POS_TABLE = 10,     /* buffer [1,n_position,D] -> first dims[0] rows [frames,D] */
    EG_PACK_LINEAR_T = 11,      /* nn.Linear weight [N,K] -> transposed [K,N] */
    EG_PACK_LINEAR_FOLD = 12,   /* key = chain "last@...@first" of nn.Linear prefixes with only Dropout between them (eval mode: an
                                   affine chain): W = W_last ... W_first folded in float64, packed as EG_PACK_LINEAR (same dims);
                                   several chains joined by '|' are concatenated along N */
    EG_PACK_BIAS_FOLD = 13,     /* the folded chain's bias, zero padded to dims[1] */
    EG_PACK_CONV1X1_BF16 = 14,  /* Conv2d [O,I,1,1] -> bf16 images [I/8][O][8], hi = bf16(w) then lo = bf16(w - hi): the 3x3 images' packing with a
                                   single tap (dims = O,I; numel = O*I floats).  I % 32 == 0, O % 16 == 0 */
    EG_PACK_WN_TAPS = 15        /* key = "<prefix>.weight_g|<prefix>.weight_v" of a weight-norm conv, kernel size 2: both taps of g*v/||v|| side by side along K, [O][tap 0 | tap 1] with
                                   each tap zero padded to Ipad, packed as EG_PACK_LINEAR with K = 2*Ipad (dims = O,I,Opad,Ipad;
                                   numel = 4*Opad*Ipad floats): the weight of eg_linear_presplit_causal */
} EgPackKind;

typedef struct EgWeightEntry {
    char key[192];              /* reference state_dict key (or module prefix for BN / weight-norm kinds) */
    int32_t kind;               /* EgPackKind */
    int32_t dims[4];
    int64_t offset;             /* floats from arena base; 64-byte aligned */
    int64_t numel;              /* packed size in floats */
} EgWeightEntry;

/* ------------------------------------------------------------------------------------------
 * Generator = Transformer (Full_model/Models_spatial_memory.py:471-616, Full_model/Models_memory.py:426-565)
 * ------------------------------------------------------------------------------------------ */
typedef struct EgGeneratorConfig {
    int32_t frames;             /* Transformer(frames=...)       :475 */
    int32_t pose_dim;           /* pose_dim                       :475 */
    int32_t prior_frames;       /* prior_frames                   :475 */
    int32_t chunk;              /* args.chunk                     :263 */
    int32_t d_model;            /* must be 512-class: multiple of 64 */
    int32_t d_inner;
    int32_t n_layers;
    int32_t n_head;
    int32_t d_k;                /* == d_v */
    int32_t n_mels;             /* spectrogram rows (128) */
    int32_t spec_len;           /* spectrogram columns (124 for 4 s) */
    int32_t text_len;           /* 60 (Linear(60,60), :164-166) */
    int32_t n_words;            /* lang_model.n_words */
    int32_t embed_dim;          /* args.wordembed_dim (300) */
    int32_t tcn_hidden;         /* args.hidden_size (300) */
    int32_t tcn_layers;         /* args.n_layers (3) */
    int32_t variant;            /* 0 = Models_spatial_memory (SP_v2 no-op), 1 = Models_memory (SP_v1 + TM) */
    int32_t precision;          /* EgPrecision */
    int32_t n_position;         /* rows of the positional table held in the checkpoint (>= frames) */
    int32_t reserved[5];        /* [0] keep_taps  [1] branch streams  [2] fold_affine: fold the Dropout-only Linear chains
                                   (post_projector :528-536, emotion_proj / semantic_proj :488-496,509-517, post_header :360-364,
                                   audio fc1 -> fc2 :128-130) into one product each at pack time -- exact algebra in eval mode,
                                   different rounding, fewer FLOPs than the reference graph: OFF for parity runs
                                   [3] 1 = keep the SE tail of identity blocks as a separate pass (default 0: gate from conv1's output
                                   moments + relu(y*gate + x) in conv2's epilogue, eg_se_gate_pre / eg_conv3x3_se)
                                   [4] 1 = the caller keeps several batches in flight on this GPU (ClipPipeline lanes): the pre-split products
                                   take the 128 x 128 tile from 64 workgroups up (less CU time, more latency); 0 = tile for stand-alone latency */
} EgGeneratorConfig;

typedef struct EgGenerator EgGenerator;

int eg_generator_default_config(EgGeneratorConfig* cfg);          /* TED: 34/126/4, spec 128x124 */
int eg_generator_create(const EgGeneratorConfig* cfg, EgGenerator** out);
void eg_generator_destroy(EgGenerator* g);
int64_t eg_generator_arena_floats(const EgGenerator* g);
int32_t eg_generator_num_weights(const EgGenerator* g);
int eg_generator_weight_entry(const EgGenerator* g, int32_t index, EgWeightEntry* out);
int64_t eg_generator_workspace_bytes(const EgGenerator* g, int32_t batch);

/* Transformer.forward (Models_spatial_memory.py:566-616 / Models_memory.py:521-565), eval mode.
 *   spec      [B, n_mels, spec_len] fp32 (dB)           text  [B, text_len] int64
 *   prior     [B, prior_frames, pose_dim]               sampled [B, frames, d_model] or NULL
 * outputs (any may be NULL to skip the copy-out; the computation is still performed):
 *   pose [B, frames, pose_dim]   emotion_feature, semantic_feature [B, frames, d_model]
 *   emotion_prediction [B, 8]    text_embedding [B, text_len, 512]                      */
int eg_generator_forward(const EgGenerator* g, const float* arena, int32_t batch,
                         const float* spec, const int64_t* text, const float* prior, const float* sampled,
                         float* pose, float* emotion_feature, float* semantic_feature,
                         float* emotion_prediction, float* text_embedding,
                         void* workspace, int64_t workspace_bytes, void* stream);

/* Diversity sampling (BASELINE config 5): the audio/semantic tower is run once per clip, then
 * fusion -> encoder -> decoder -> post_projector for `draws` sampled emotion maps per clip.
 *   sampled [B, draws, frames, d_model]    pose [B, draws, frames, pose_dim]               */
int eg_generator_forward_draws(const EgGenerator* g, const float* arena, int32_t batch, int32_t draws,
                               const float* spec, const float* prior, const float* sampled, float* pose,
                               void* workspace, int64_t workspace_bytes, void* stream);
int64_t eg_generator_draws_workspace_bytes(const EgGenerator* g, int32_t batch, int32_t draws);

/* Long-form synthesis: W consecutive windows of U utterances rolled out on the device.  Window 0 is seeded with seed_pose; window
 * w >= 1 with the RAW last prior_frames poses of window w-1 (never the blended track).  Every step sees the U windows of index w as
 * one batch (the memory variant's TM_Memory_Net couples the utterances of a step, never the windows of an utterance).
 * With F = frames, P = prior_frames, H = F - P, D = pose_dim:
 *   spec   [U, W, n_mels, spec_len]     text [U, W, text_len] int64 (may be NULL unless text_embedding is wanted)
 *   seed_pose [U, P, D]                 sampled [U, W, F, d_model] or NULL (the generator's own emotion feature, as in forward)
 *   alpha  [P] overlap weights on the device, or NULL for alpha[j] = (j + 1) / (P + 1)
 *   track  [U, W*H + P, D]:  rows [0, F) = pose_0;  for w >= 1 row w*H + j = (1 - alpha[j]) * pose_{w-1}[H + j] + alpha[j] * pose_w[j]
 *          for j < P (two rounded products, one rounded sum) and pose_w[j] for P <= j < F
 *   optional (NULL to skip): windows [U, W, F, D] raw per-window poses, emotion_prediction [U, W, 8],
 *          emotion_feature / semantic_feature [U, W, F, d_model], text_embedding [U, W, text_len, 512]
 * Two phases on `stream`, no allocation, host round trip or synchronisation (capturable into one hipGraph for fixed U, W):
 *   A, batch U*W in window-major order: text branch (only when text_embedding is wanted), audio tower, projections, classifier header,
 *      fusion, encoder, and every decoder layer's K|V projection of the encoder output, kept as fp32 (what the attention kernel reads);
 *   B, W steps of U clips: prior encoder -> decoder layers over the step's K|V slice -> post_projector -> one hand-off launch that
 *      writes track, windows[:, w] and the next step's prior.
 * Requires utterances >= 1, windows >= 1, n_layers <= 8, utterances * windows <= 2^20.  fold_affine generators are supported (the folded
 * products are used in both phases).  The branch streams of `concurrent` generators are not used: everything is enqueued on `stream`.
 * Phase B takes the product paths eg_generator_forward takes at batch U (the one-clip split-K of w_2 included); phase A takes those of
 * batch U*W, so against a loop of eg_generator_forward calls the result is bitwise equal where the products are chunking-invariant
 * (U >= 2) and equal to rounding at U == 1. */
int eg_generator_forward_rollout(const EgGenerator* g, const float* arena, int32_t utterances, int32_t windows,
                                 const float* spec, const int64_t* text, const float* seed_pose, const float* sampled,
                                 const float* alpha, float* track, float* windows_out, float* emotion_prediction,
                                 float* emotion_feature, float* semantic_feature, float* text_embedding,
                                 void* workspace, int64_t workspace_bytes, void* stream);
int64_t eg_generator_rollout_workspace_bytes(const EgGenerator* g, int32_t utterances, int32_t windows);

/* Diverse roll-out: R = draws sampled tracks for each of U recordings in one call.  By definition the result is
 * eg_generator_forward_rollout on U*R recordings, recording u*R + r having spec[u], text[u], seed_pose[u] and sampled[u, r]:
 *   spec [U, W, n_mels, spec_len]   text [U, W, text_len] int64 (may be NULL unless text_embedding is wanted)   seed_pose [U, P, D]
 *   sampled [U, R, W, F, d_model], REQUIRED (without it every draw would be the same track)        alpha [P] or NULL
 *   track [U, R, W*H + P, D];  optional: windows [U, R, W, F, D], and -- independent of the draw, returned once --
 *   emotion_prediction [U, W, 8], emotion_feature / semantic_feature [U, W, F, d_model], text_embedding [U, W, text_len, 512]
 * The sampled map enters the generator at the fusion input (Models_spatial_memory.py:601-602 / Models_memory.py:551-552) and the prior
 * through the prior encoder -> decoder target stream only (:585, :611 / :535, :560), so the text branch, the audio tower, the projections
 * and the classifier header (:577-592 / :527-542) see neither the draw nor the prior:
 *   A: tower side at batch N = U*W in clip order n = w*U + u -- the launches eg_generator_forward_rollout makes at batch N; ONE fusion
 *      launch (draws.hip) writes fus_in[(w*U + u)*R + r] = sampled[u, r, w] + semantic[w*U + u], reading the caller's order (no
 *      window-major copy of `sampled`); encoder and every decoder layer's K|V product at N*R sequences;
 *   B: W steps at batch U*R: prior encoder -> decoder over the step's contiguous K|V slice -> post_projector -> the roll-out's hand-off
 *      kernel with U*R rows (the same handoff_blend).  Row u*R + r of a step is row u*R + r of track viewed [U*R, T, D]; in the memory
 *      variant TM_Memory_Net couples the U*R rows of a step, as in the replicated call.  Step 0's prior is seed_pose[u] repeated over
 *      the R draws by one launch of U*R*P*D elements (not by indexing row / R where the seed is read).
 * Same contract as eg_generator_forward_rollout: one stream, no allocation, host round trip or synchronisation; launches, grids and
 * pointers are fixed for fixed (U, W, R): capturable into one hipGraph.  Fusion, encoder, K|V and phase B run at the batch of the
 * replicated call, and the tower-side products accumulate K in one order from two clips up, so for U*W >= 2 every output equals the
 * replicated eg_generator_forward_rollout bit for bit (f32 and bf16x3); at U*W == 1 the tower side takes the one-clip paths (split-K of
 * w_2, the one-clip convolution tiles) where the replicated call has R clips: equal to rounding.  With draws == 1 the call IS
 * eg_generator_forward_rollout (its launches, its bits).
 * Refuses by name, before the first launch: a null required pointer (sampled included), utterances / windows / draws < 1,
 * utterances*windows*draws > 2^20, n_layers > 8, text_embedding without text, a short workspace, buffers not 16-byte aligned.
 * workspace >= eg_generator_rollout_draws_workspace_bytes, which is 0 for arguments the call would refuse and equals
 * eg_generator_rollout_workspace_bytes(g, U, W) at draws == 1. */
int eg_generator_forward_rollout_draws(const EgGenerator* g, const float* arena, int32_t utterances, int32_t windows, int32_t draws,
                                       const float* spec, const int64_t* text, const float* seed_pose, const float* sampled,
                                       const float* alpha, float* track, float* windows_out, float* emotion_prediction,
                                       float* emotion_feature, float* semantic_feature, float* text_embedding,
                                       void* workspace, int64_t workspace_bytes, void* stream);
int64_t eg_generator_rollout_draws_workspace_bytes(const EgGenerator* g, int32_t utterances, int32_t windows, int32_t draws);

/* Ragged roll-out: the roll-out above for U recordings with their OWN window counts W_u >= 1 (N = sum W_u, Wmax = max W_u), in one call.
 * Step s (0 <= s < Wmax) is the generator on the ACTIVE recordings {u : W_u > s}, taken in the working order "longer first, ties by
 * index" (stable sort by (-W_u, u)): the active set of every step is a prefix of that order, the batch of step s is U_s = #{u : W_u > s},
 * and nothing of an inactive recording enters a step (the memory variant's TM_Memory_Net couples exactly the active recordings).
 * Recording u's window w >= 1 is seeded with the raw last P poses of its own window w-1, window 0 with seed_pose[u]; its track is the
 * stitch of its own W_u windows.  Arguments and results are in the CALLER's recording order.
 *
 * The plan (host only: no HIP call, usable without a GPU).  From windows_per [U] it fills (any output may be NULL):
 *   order [U]       rank -> recording, the working order          inverse [U]    recording -> rank
 *   step_batch [Wmax]   U_s, non-increasing, sums to N
 *   table [N + 2U] (the count eg_rollout_ragged_plan_ints returns), what the device reads:
 *       [0, N)       slot_row: step-major slot (s, rank) = sum_{s' < s} U_s' + rank  ->  packed row off[order[rank]] + s,
 *                    off = exclusive prefix sum of W_u in caller order (a permutation of 0 .. N-1)
 *       [N, N+U)     order           [N+U, N+2U)  W_order[rank]
 * The caller uploads `table` once per (W_u) vector as int32 and passes the device copy as `plan`, beside the host array windows_per.
 * Refuses utterances < 1, W_u < 1 and N > 2^20 by name.  eg_rollout_ragged_plan_ints is 0 for counts it would refuse. */
/* Whole rows moved by an index table on the device (the ragged roll-out's gather / scatter; also packs padded [U, Wmax, ...] arguments):
 *   scatter == 0: out[i] = in[d_table[i]]      scatter != 0: out[d_table[i]] = in[i]      for i < rows,
 * rows of row_words 32-bit words, d_table int32 [rows] on the device; 16-byte accesses when row_words % 4 == 0 and both buffers are
 * 16-byte aligned.  The table entry is read once per row.  The entries are the caller's: they must index rows that exist, and for a scatter be
 * distinct.  One launch. */
int eg_rows_by_table(const void* in, void* out, const int32_t* d_table, int32_t rows, int64_t row_words, int32_t scatter, void* stream);
int64_t eg_rollout_ragged_plan_ints(int32_t utterances, int64_t total_windows);
int eg_rollout_ragged_plan(const int32_t* windows_per, int32_t utterances, int32_t* order, int32_t* inverse, int32_t* step_batch,
                           int32_t* table);
/* With F, P, H, D as above, every window-indexed array PACKED recording-major: recording u owns rows [off[u], off[u] + W_u):
 *   windows_per [U] on the HOST        plan [N + 2U] int32 on the DEVICE (the plan's table for the same windows_per)
 *   spec [N, n_mels, spec_len]         text [N, text_len] int64 (may be NULL unless text_embedding is wanted)
 *   seed_pose [U, P, D]                sampled [N, F, d_model] or NULL      alpha [P] on the device or NULL
 *   track [U, Wmax*H + P, D]: rows [0, W_u*H + P) of recording u as eg_generator_forward_rollout defines them (the same blend: two
 *          rounded products, one rounded sum); rows [W_u*H + P, Wmax*H + P) are ZERO, written by this call
 *   optional (NULL to skip): windows [N, F, D], emotion_prediction [N, 8], emotion_feature / semantic_feature [N, F, d_model],
 *          text_embedding [N, text_len, 512]
 * Same contract as eg_generator_forward_rollout: one stream, no allocation on the device, host round trip or synchronisation; for a fixed
 * (W_u) vector the launches, grids and pointers are fixed, so the call captures into one hipGraph.
 *   A, batch N in step-major order: the packed inputs are brought into it by one row gather each through slot_row (16-byte accesses where
 *      the row length allows; skipped when U == 1 or Wmax == 1, where the two orders coincide), then the launches of phase A above; the
 *      wanted per-window outputs go back to packed rows by one row scatter each.  Step s's K|V is the contiguous slice of its U_s slots.
 *   B, Wmax steps at batch U_s: prior encoder -> decoder -> post_projector (the product paths eg_generator_forward takes at batch U_s)
 *      -> one hand-off launch for the active ranks: track rows, windows, and the next prior into ping-pong buffers indexed by RANK (a
 *      recording keeps its slot for its whole life).  The zero fill of a recording's track tail is folded into that recording's LAST
 *      hand-off (no launch of its own).  The seed poses are gathered into rank order by one launch unless they already are in it.
 * With every W_u equal the call makes exactly the launches of eg_generator_forward_rollout on that rectangle and returns its results bit
 * for bit.  workspace >= eg_generator_rollout_ragged_workspace_bytes at (U, N): a function of U and N only, equal to
 * eg_generator_rollout_workspace_bytes at (U, W) when N = U*W -- the plan table is the caller's buffer, not workspace.  It is 0 for
 * utterances < 1, N < utterances, N > 2^20, n_layers > 8.  Refused by name before the first launch: utterances < 1, W_u < 1, N > 2^20, n_layers > 8, a
 * short workspace, null pointers, misaligned buffers. */
int eg_generator_forward_rollout_ragged(const EgGenerator* g, const float* arena, int32_t utterances, const int32_t* windows_per,
                                        const int32_t* plan, const float* spec, const int64_t* text, const float* seed_pose,
                                        const float* sampled, const float* alpha, float* track, float* windows_out,
                                        float* emotion_prediction, float* emotion_feature, float* semantic_feature, float* text_embedding,
                                        void* workspace, int64_t workspace_bytes, void* stream);
int64_t eg_generator_rollout_ragged_workspace_bytes(const EgGenerator* g, int32_t utterances, int64_t total_windows);

/* Takes: R sampled tracks for each of U recordings with their OWN window counts W_u -- the general roll-out, of which the ragged call
 * (R == 1) and the diverse call (every W_u equal) are special cases.  By definition eg_generator_forward_rollout_ragged on U*R recordings,
 * recording u*R + r having recording u's spec windows, text, seed pose and W_u, and its own sampled maps: the replication rule
 * eg_generator_forward_rollout_draws has against eg_generator_forward_rollout.  With N = sum W_u, off the exclusive prefix sum of W_u:
 *   windows_per [U] on the HOST        plan [2N + 2U] int32 on the DEVICE (eg_rollout_takes_plan's table for the same windows_per)
 *   spec [N, n_mels, spec_len], text [N, text_len] int64 (may be NULL unless text_embedding is wanted): packed recording-major, as for
 *          eg_generator_forward_rollout_ragged         seed_pose [U, P, D]: one per recording        alpha [P] on the device or NULL
 *   sampled [N*R, F, d_model] (required): the packed order of the replicated ragged call -- recording u owns rows
 *          [R*off[u], R*off[u] + R*W_u), window w of draw r is row R*off[u] + r*W_u + w
 *   track [U, R, Wmax*H + P, D]: rows [0, W_u*H + P) of track[u, r] as the ragged call defines them, the rest ZERO, every element written
 *   optional (NULL to skip): windows [N*R, F, D] in the order of `sampled`; independent of the draw and returned once, packed:
 *          emotion_prediction [N, 8], emotion_feature / semantic_feature [N, F, d_model], text_embedding [N, text_len, 512]
 * The takes plan (host only, like eg_rollout_ragged_plan and with its arguments): table [2N + 2U] (eg_rollout_takes_plan_ints; 0 for
 * counts the plan refuses) = eg_rollout_ragged_plan's table [N + 2U], then slot_rank [N]: the rank of step-major slot (s, rank).
 * The R copies of a recording tie in the replicated call's working order and keep their index order, so its rank is rank*R + r and its
 * slot is slot*R + r:
 *   A: the ragged call's phase A at batch N (tower side, text, heads: once per window); ONE fusion launch (draws.hip) writes
 *      fus_in[slot*R + r] = sampled[R*off + r*W_u + s] + semantic[slot], looking rank, off, W_u and s up in the table; encoder and every
 *      decoder layer's K|V product at N*R sequences;
 *   B: Wmax steps at batch U_s*R, row rank*R + r: prior encoder -> decoder over the step's contiguous K|V slice (U_s*R slots) ->
 *      post_projector -> one hand-off launch (draws.hip: track[u, r] rows, windows, the next prior by row, and in a recording's LAST step
 *      the zero fill of its R track tails).  Step 0's prior is seed_pose[order[rank]] repeated over the R draws by one launch.
 * Same contract as the calls above: one stream, no allocation, host round trip or synchronisation; launches, grids and pointers are fixed
 * for a fixed (W_u) vector and R: capturable into one hipGraph.  Fusion, encoder, K|V and phase B run at the batch and row order of the
 * replicated call and the tower-side products accumulate K in one order from two clips up, so for N >= 2 every output equals the replicated
 * ragged call bit for bit; at N == 1 the tower side takes the one-clip paths where the replicated call has R clips: equal to rounding.
 * With draws == 1 the call IS eg_generator_forward_rollout_ragged (its launches, its bits); with every W_u equal it returns
 * eg_generator_forward_rollout_draws's track bit for bit.
 * Refuses by name, before the first launch: a null required pointer (sampled included), utterances / draws / W_u < 1, N > 2^20 or
 * N*draws > 2^20, n_layers > 8, text_embedding without text, a short workspace, buffers not 16-byte aligned (plan: 4-byte).
 * workspace >= eg_generator_rollout_takes_workspace_bytes at (U, N, R): 0 for what the call refuses, equal to
 * eg_generator_rollout_draws_workspace_bytes(g, U, W, R) when N = U*W and to eg_generator_rollout_ragged_workspace_bytes(g, U, N) at
 * draws == 1 (the tower side is carved once per window: below the replicated call's eg_generator_rollout_ragged_workspace_bytes(g, U*R, N*R)). */
int64_t eg_rollout_takes_plan_ints(int32_t utterances, int64_t total_windows);
int eg_rollout_takes_plan(const int32_t* windows_per, int32_t utterances, int32_t* order, int32_t* inverse, int32_t* step_batch,
                          int32_t* table);
int eg_generator_forward_rollout_takes(const EgGenerator* g, const float* arena, int32_t utterances, int32_t draws,
                                       const int32_t* windows_per, const int32_t* plan, const float* spec, const int64_t* text,
                                       const float* seed_pose, const float* sampled, const float* alpha, float* track, float* windows_out,
                                       float* emotion_prediction, float* emotion_feature, float* semantic_feature, float* text_embedding,
                                       void* workspace, int64_t workspace_bytes, void* stream);
int64_t eg_generator_rollout_takes_workspace_bytes(const EgGenerator* g, int32_t utterances, int64_t total_windows, int32_t draws);

/* Streaming synthesis: the roll-out fed hop by hop.  A session of `rows` = U rows lives in a caller-owned device buffer `state`
 * (eg_stream_state_bytes, 16-byte aligned, carved deterministically from (g, rows, hop_samples, n_samples): pass the same four to every
 * entry): an audio ring [U, lag * hop], lag = ceil(n_samples / hop_samples), the prior [U, P, D] and per row the counters c (pushes since
 * the row's reset), w (windows done), total (-1 while the row is open, else the number of samples T the row was fed) and the verdict of
 * the last push.  The counters stay on the device: no entry reads them back, every entry is stream-ordered and makes no allocation,
 * synchronisation or host round trip, and the launches, grids and pointers of push and step do not depend on the step index, so one
 * captured hipGraph of push (-> eg_melspectrogram -> eg_cvae_sample) -> step serves a stream for ever.
 * With F = frames, P = prior_frames, H = F - P, D = pose_dim, hop = hop_samples, n = n_samples:
 *   open row:   window w = samples [w*hop, w*hop + n) of the row's recording; ready when c >= w + lag (it then starts at the oldest
 *               sample the ring holds; samples before the start of the recording are zero).
 *   ended row:  window w is ready while w*hop < total; it holds L = total - w*hop real samples and, if L < n, is completed by symmetric
 *               padding of its own samples (period 2L, np.pad mode="symmetric": eg_window_gather's rule).
 * A row's emitted rows, concatenated and followed by its tail, are the track eg_generator_forward_rollout returns for the same recording
 * [:T] with W = the number of windows taken. */
int64_t eg_stream_state_bytes(const EgGenerator* g, int32_t rows, int32_t hop_samples, int32_t n_samples);
/* Rows with row_mask[u] != 0 (device int32 [U]; NULL: every row): c = w = 0, total = -1, ring row zeroed, prior := seed_pose[u]
 * (seed_pose [U, P, D]; the rows not selected are not read). */
int eg_stream_reset(const EgGenerator* g, void* state, int32_t rows, int32_t hop_samples, int32_t n_samples,
                    const int32_t* row_mask, const float* seed_pose, void* stream);
/* One step of audio for every row: chunk [U, hop] is written into the ring with wrap-around (nothing is moved), c += 1, and a row with
 * ends[u] = m in [0, hop] (device int32 [U], -1 = the row goes on; NULL: all go on) ends here: only its first m samples are real, total =
 * (c - 1)*hop + m.  That push and every later one is still a step for an ended row: its audio is ignored and its ring is fed zeros.
 * clips [U, n]: every row's window w, oldest sample first, by the rules above -- bitwise eg_window_gather's clip on the same recording;
 * a row without a ready window (waiting for its first `lag` pushes, or ended and out of windows) gets an ALL-ZERO clip, whose
 * eg_melspectrogram is finite: 0 dB throughout (power_to_db's amin 1e-10 is both the value and the reference), |value| < 1e-6 after
 * the fp16 rounding.  Two launches.  Call eg_generator_stream_step at most once per push: a second step would emit the window again. */
int eg_stream_push(const EgGenerator* g, void* state, int32_t rows, int32_t hop_samples, int32_t n_samples, const float* chunk,
                   const int32_t* ends, float* clips, void* stream);
/* The launches of eg_generator_forward at batch U on `stream` with the prior read from the state (the product paths eg_generator_forward
 * takes at batch U, the one-clip split-K included; workspace >= eg_generator_workspace_bytes(g, U); the branch streams of `concurrent`
 * generators are not used), then ONE hand-off launch that applies, per row, the verdict of the last eg_stream_push:
 *   ready:      rows_out[u] = track rows [w*H, (w+1)*H): for w >= 1 the first P are (1 - alpha[j]) * prior[u, j] + alpha[j] * pose[u, j]
 *               (two rounded products, one rounded sum: the roll-out's blend, one device function), the rest the raw pose;
 *               prior[u] := pose[u, H:F] (raw), w += 1, valid_out[u] = 1, window_out[u] = pose[u]
 *   not ready:  rows_out[u] = 0, window_out[u] = 0, valid_out[u] = 0; prior and w unchanged.
 *   spec [U, n_mels, spec_len]   text [U, text_len] int64 or NULL (the text branch does not reach the pose: NULL skips it)
 *   sampled [U, F, d_model] or NULL   alpha [P] on the device or NULL for (j + 1) / (P + 1)
 *   rows_out [U, H, D]   valid_out [U] int32   optional (NULL to skip): window_out [U, F, D], emotion_prediction [U, 8]
 * The prior is read and overwritten in that launch at its fixed address, each element by one thread.  The memory variant's TM_Memory_Net
 * couples the rows of a step: there every row's result depends on the priors of ALL rows, ready or not. */
int eg_generator_stream_step(const EgGenerator* g, const float* arena, void* state, int32_t rows, int32_t hop_samples,
                             int32_t n_samples, const float* spec, const int64_t* text, const float* sampled, const float* alpha,
                             float* rows_out, int32_t* valid_out, float* window_out, float* emotion_prediction,
                             void* workspace, int64_t workspace_bytes, void* stream);
/* out [U, P, D] = the priors: the last P rows of every row's track as it stands. */
int eg_stream_tail(const EgGenerator* g, const void* state, int32_t rows, int32_t hop_samples, int32_t n_samples, float* out,
                   void* stream);

/* Intermediate taps of the most recent eg_generator_forward on this workspace (for parity tests):
 * returns the device pointer inside `workspace` and the element count; names: "stem", "layer1", "layer2", "layer3"
 * (NHWC, only when the generator was created with keep_taps), "audio_map", "audio_feat", "prior_enc", "fusion", "enc_out",
 * "dec_out", and the buffers the attention blocks reuse -- contents of the LAST block that ran: "attn_q", "attn_qkv",
 * "attn_out", "mha_out", "proj". */
int eg_generator_tap(const EgGenerator* g, int32_t batch, void* workspace, const char* name,
                     float** d_ptr, int64_t* numel);

/* ------------------------------------------------------------------------------------------
 * Emotion CVAE = MLP_Reconstruct_v3 (CAVE/BEAT_CVAE.py:312-460)
 * ------------------------------------------------------------------------------------------ */
typedef struct EgCvaeConfig {
    int32_t frames;             /* decoder output channels; 60 hard-coded upstream (:365-368) */
    int32_t d_model;            /* 512 = 4 * latent map width 128 (:445) */
    int32_t latent;             /* 32 */
    int32_t n_classes;          /* 8 */
    int32_t reserved[4];
} EgCvaeConfig;
typedef struct EgCvae EgCvae;

int eg_cvae_default_config(EgCvaeConfig* cfg);
int eg_cvae_create(const EgCvaeConfig* cfg, EgCvae** out);
void eg_cvae_destroy(EgCvae* c);
int64_t eg_cvae_arena_floats(const EgCvae* c);
int32_t eg_cvae_num_weights(const EgCvae* c);
int eg_cvae_weight_entry(const EgCvae* c, int32_t index, EgWeightEntry* out);
int64_t eg_cvae_workspace_bytes(const EgCvae* c, int32_t n);

/* MLP_Reconstruct_v3.sample (:427-447).  y [n, 8] one-hot, z [n, 32] latent draw (the host draws it
 * with torch.randn on the CPU generator exactly as :441 does) -> out [n, frames, d_model]. */
int eg_cvae_sample(const EgCvae* c, const float* arena, int32_t n, const float* y, const float* z,
                   float* out, void* workspace, int64_t workspace_bytes, void* stream);
/* MLP_Reconstruct_v3.forward (:403-424), eval-mode BN.  x [n, frames, d_model], y [n,8], eps [n,32]
 * (reparameterize :389-399: z = eps*exp(0.5*logvar)+mu) -> recon [n, frames, d_model], mu, logvar [n,32]. */
int eg_cvae_forward(const EgCvae* c, const float* arena, int32_t n, const float* x, const float* y,
                    const float* eps, float* recon, float* mu, float* logvar,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mel front-end = extract_melspectrogram (utils/train_utils_BEAT.py:186-190) + the loader's
 * column slice (data_loader/lmdb_loader_BEAT_full.py:229)
 * ------------------------------------------------------------------------------------------ */
/* audio [B, n_samples] fp32 16 kHz -> spec [B, 128, out_frames] fp32 holding fp16-rounded dB.
 * n_fft 1024, hop 512, centred (zero pad), periodic Hann, 128 Slaney mels, power_to_db(ref=max, top_db=80).
 * d_melfb_t [513,128] (transposed filterbank), d_window [1024], d_twiddle [512,2], d_band [128,2] are caller-provided
 * device copies of the tables eg_mel_tables fills on the host.
 * workspace >= eg_mel_workspace_bytes.
 * EG_MEL_FFT (read per call): unset, empty or "4" = the register radix-4 transform; "2" = the radix-2 LDS transform it replaces (A/B runs);
 * any other value is EG_ERR_BAD_ARG before any launch. */
int eg_mel_tables(float* h_melfb_t /*513*128, transposed*/, float* h_window /*1024*/, float* h_twiddle /*2*512*/,
                  int32_t* h_band /*128*2: non-zero bin range of each mel filter*/);
int64_t eg_mel_workspace_bytes(int32_t batch, int32_t n_samples);
int eg_melspectrogram(const float* audio, int32_t batch, int32_t n_samples, const float* d_melfb_t,
                      const float* d_window, const float* d_twiddle, const int32_t* d_band, float* spec, int32_t out_frames,
                      void* workspace, int64_t workspace_bytes, void* stream);
/* Overlapping windows of long recordings as a batch of clips, for eg_melspectrogram (each window is its own clip: centre padding and
 * power_to_db(ref=max) are per clip upstream, so windows cannot share STFT frames):
 *   audio [utterances, total_samples] -> out [utterances * windows, n_samples], out[u*W + w, i] = audio[u, w*hop_samples + i],
 * A window that runs past the end of the track is completed from its own L = total_samples - w*hop_samples samples as
 * make_audio_fixed_length does (utils/train_utils_BEAT.py:220-226, np.pad mode="symmetric": mirrored about the end, period 2L).
 * Every window must start inside the track: (windows - 1) * hop_samples < total_samples. */
int eg_window_gather(const float* audio, int32_t utterances, int64_t total_samples, int32_t windows, int64_t hop_samples,
                     int32_t n_samples, float* out, void* stream);
/* The same for recordings of unequal length: audio [utterances, stride], recording u holds lengths[u] real samples (1 .. stride; what
 * follows them in its row is never read) and has W_u = ceil(lengths[u] / hop_samples) windows -- every window that starts inside the
 * recording (w * hop_samples < lengths[u]), the rule eg_stream_push states for an ended row, so a stream and the offline path count the
 * same windows.  out [N, n_samples], N = sum W_u, packed recording-major: row off[u] + w is eg_window_gather's clip for a recording of
 * lengths[u] samples (a window that runs past the recording's own end is completed by symmetric padding of its own L = lengths[u] -
 * w*hop_samples samples).  lengths [U] int64 on the HOST (checked here); d_meta [2U] int64 on the DEVICE: lengths [U] | off [U], the
 * caller's upload of the same numbers.  Refuses utterances < 1, lengths[u] < 1 or > stride, and N > 2^20 by name.  One launch. */
int eg_window_gather_ragged(const float* audio, int32_t utterances, int64_t stride, const int64_t* lengths, const int64_t* d_meta,
                            int64_t hop_samples, int32_t n_samples, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Polyphase resampler: audio at rate_in -> the model's rate_out (16000) on the device (csrc/resample.hip)
 * ------------------------------------------------------------------------------------------ */
/* g = gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g; supported: max(L, M) <= EG_RESAMPLE_MAX_FACTOR (8000, 11025, 12000, 22050,
 * 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000 -> 16000 among them); anything else is refused with its L and M.
 * Filter: half = 10 * max(L, M), 2*half + 1 taps, fc = 1 / max(L, M), h[k] = fc * sinc(fc * (k - half)) * kaiser(beta 5)[k], normalised to
 * sum 1, times L: scipy.signal.firwin(2*half + 1, fc, window=("kaiser", 5.0)) * L, the filter of scipy.signal.resample_poly's defaults,
 * designed in float64 on the host and rounded to fp32.
 * Output: n_out = ceil(n_in * L / M), y[n] = sum_i x[i] * h[half + (n - delay)*M - i*L] over 0 <= i < n_in with the tap index inside
 * [0, 2*half]; delay = 0 is resample_poly(x, L, M).  x outside [0, n_in) is zero and is never read.
 * K = ceil((2*half + 1) / L) taps per output; the device table is the polyphase bank [L][pitch], pitch = K | 1 (odd: consecutive phases start
 * in different LDS banks), bank[phase][j] = h[phase + j*L], zero past the last tap and in the pad column.
 * Streaming: output n needs half / L future inputs, so a stream's signal is the offline one delayed by D = ceil(half / M) output samples,
 * y_d[n] = y[n - D], cut to ceil(n_in * L / M) samples; the history a push needs is the last Hs = ceil((D*M + half) / L) input samples.
 * eg_resample_plan, eg_resample_out_length (-1 for refused arguments) and eg_resample_filter are host only: no HIP call, usable without a
 * GPU.  eg_resample_filter fills h_taps [2*half + 1] and / or h_bank [bank_floats] (either may be NULL, not both). */
#define EG_RESAMPLE_MAX_FACTOR 640
#define EG_RESAMPLE_TILE 1024       /* output samples of one workgroup of the offline kernel */
typedef struct EgResamplePlan {
    int32_t L, M, half, K, D, Hs;
    int32_t pitch;              /* floats per phase row of the bank */
    int32_t bank_floats;        /* L * pitch */
} EgResamplePlan;
int eg_resample_plan(int32_t rate_in, int32_t rate_out, EgResamplePlan* plan);
int64_t eg_resample_out_length(int64_t n_in, int32_t rate_in, int32_t rate_out);
int eg_resample_filter(int32_t rate_in, int32_t rate_out, float* h_taps, float* h_bank);
/* Offline: x [U, in_stride], row u holds lengths[u] real samples (1 .. in_stride; what follows them may be anything, NaN included) ->
 * y [U, out_stride]: row u's ceil(lengths[u] * L / M) samples of the signal delayed by `delay` >= 0 output samples, then zeros up to
 * out_stride (>= the longest row's output).  lengths [U] int64 on the HOST (checked here), d_lengths [U] int64 on the DEVICE: the caller's
 * upload of the same numbers; d_bank: device copy of eg_resample_filter's bank.  One launch, grid (output tile of EG_RESAMPLE_TILE, row),
 * one owning thread per output element, no atomics; the input span of a tile is staged in LDS (16-byte loads where x is 16-byte aligned
 * and in_stride % 4 == 0).  A row's result does not depend on U, on its place in the batch or on the strides.  Launch, grid and pointers
 * depend on (U, strides, rates) only: the call captures into a hipGraph.  Refuses by name before the launch: null pointers, y / d_bank not
 * 16-byte aligned, rates, U outside 1 .. 65535, lengths[u] outside 1 .. in_stride, a short out_stride, delay < 0. */
int eg_resample(const float* x, int32_t rows, int64_t in_stride, const int64_t* lengths, const int64_t* d_lengths, int32_t rate_in,
                int32_t rate_out, const float* d_bank, int64_t delay, float* y, int64_t out_stride, void* stream);
/* Stream: state = the history [rows, Hs] fp32 in a caller-owned device buffer of eg_resample_stream_state_bytes (0 for refused arguments).
 * eg_resample_stream_reset zeroes the history of the rows with row_mask[u] != 0 (device int32 [rows]; NULL: every row).
 * eg_resample_stream_push: chunk_in [rows, hop_in] + ends_in (device int32 [rows]; -1: the row goes on, else the number of real samples in
 * this chunk -- what follows them is never read; NULL: all go on) -> out [rows, hop_out]: the next hop_out samples of the delayed signal;
 * a row that ends with m real samples has ceil(m * L / M) real output samples in this push and zeros after them.  hop_in must be
 * hop_out * M / L exactly (then every push is the same computation on [history | chunk] in local indices: no device counter, nothing
 * depends on the step index) and >= Hs.  Two launches: the outputs, then the new history (the last Hs samples of the chunk, zero from the
 * row's end on) in a launch of its own, so no launch reads and overwrites the history.  The outputs come from the device function the
 * offline kernel uses: the pushes of a recording, concatenated, are eg_resample(delay = D) on it bit for bit. */
int64_t eg_resample_stream_state_bytes(int32_t rows, int32_t rate_in, int32_t rate_out);
int eg_resample_stream_reset(void* state, int32_t rows, int32_t rate_in, int32_t rate_out, const int32_t* row_mask, void* stream);
int eg_resample_stream_push(void* state, int32_t rows, int32_t rate_in, int32_t rate_out, const float* d_bank, const float* chunk_in,
                            int32_t hop_in, const int32_t* ends_in, float* out, int32_t hop_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Rows of whole tracks: what (rows, T, d_frames, draws, frame_unit [, frames]) mean in every whole-track stage below (csrc/rows.h)
 * ------------------------------------------------------------------------------------------ */
/* rows = U * draws tracks of T frames: recording u owns the `draws` consecutive rows from u * draws on.  d_frames: device int32 [rows / draws],
 * 4-byte aligned, one count per recording, or NULL; frame_unit: what one count stands for, 1 for frame counts, H for a stream's 0 / 1 valid
 * flags.  Row b has n = clamp(d_frames[b / draws] * frame_unit, 0, T) valid frames, in 64-bit (d_frames NULL: T).  Frames t >= n are never
 * used and may hold NaN; outputs behind a row's last frame are zeros.  A stage that needs a minimum of valid frames (a window, four
 * positions, one frame) cannot check a device count before its launch, so it also takes `frames`, the HOST copy of the counts (int32
 * [rows / draws]; NULL exactly when d_frames is NULL), and refuses the first recording below the minimum by name.  Nothing ties the two
 * copies together: a row whose device count is below the minimum although the host count is not comes out as zeros, and every access stays
 * in range.  Every stage refuses by name, before its first launch: d_frames not 4-byte aligned, rows not a multiple of draws (or draws < 1),
 * frame_unit < 1, `frames` and d_frames not given together, a host count below the minimum. */

/* ------------------------------------------------------------------------------------------
 * Skeleton output: tracks of bone direction vectors <-> joint positions on the device (csrc/skeleton.hip)
 * ------------------------------------------------------------------------------------------ */
/* A skeleton is a table of K bones in topological order, 1 <= K <= EG_SKELETON_MAX_BONES, over J = K + 1 joints: bone k = (parents[k],
 * children[k], lengths[k]); joint 0 is the root at the origin.  eg_skeleton_check (host only, no HIP call) refuses by name: K out of range,
 * a child that is joint 0 or outside 1..K, a child used twice, a parent that is neither the root nor the child of an earlier bone, a
 * length that is not finite and > 0.  The device copy d_table is 3K 32-bit words: parents [K] | children [K] | lengths [K] (fp32).
 * eg_skeleton_out_frames: ceil(n * L / M) for the reduced ratio L / M (-1 for refused arguments: n < 0, L or M < 1, max(L, M) after
 * reduction > EG_SKELETON_MAX_FACTOR).  eg_skeleton_tile_frames: EG_SKELETON_TILE_FRAMES. */
#define EG_SKELETON_MAX_BONES 63
#define EG_SKELETON_MAX_FACTOR 64
#define EG_SKELETON_TILE_FRAMES 32  /* output frames of one workgroup */
int eg_skeleton_check(const int32_t* parents, const int32_t* children, const float* lengths, int32_t bones);
int64_t eg_skeleton_out_frames(int64_t n, int32_t L, int32_t M);
int32_t eg_skeleton_tile_frames(void);
/* Forward: track [rows, T, 3K] fp32 -> joints [rows, out_stride, J, 3] fp32, out_stride >= ceil(T * L / M); L / M = output rate / input
 * rate (reduced here).  For a source frame t: x_k = track[b, t, 3k .. 3k+2] + d_mean[3k ..] (d_mean NULL: no mean term); unit != 0:
 * x_k /= max(|x_k|, 1e-12); p[0] = 0, p[children[k]] = p[parents[k]] + lengths[k] * x_k in table order.  Row b has
 * n valid frames ("Rows of whole tracks" above: d_frames, draws, frame_unit)
 * and n_out = ceil(n * L / M) output frames: frame k' is p(lo) + (p(lo + 1) - p(lo)) * f with lo = min(floor(k' M / L), n - 2),
 * f = (k' M - lo L) / L in exact integers (linear interpolation, extrapolated past the last frame; n = 1: p(0)); at L / M = 1 nothing is
 * blended and frame k' is p(k').  Frames k' >= n_out are written as zeros; source frames t >= n are never used and may hold NaN.
 * Inverse: joints [rows, T, J, 3] -> dir_vec [rows, T, 3K]: d = p[children[k]] - p[parents[k]], d / max(|d|, 1e-12) (a zero-length bone
 * gives the zero vector), minus d_mean when given; zeros from frame n on.
 * parents / children / lengths are on the HOST (checked here as eg_skeleton_check does), d_table is the caller's upload of the same numbers.
 * Nothing ties the upload to the host table: with a d_table that differs from it the result is unspecified (the kernels clamp its joint
 * numbers to 0..K, so the accesses stay in range).
 * All pointers are caller-owned; no allocation, no synchronisation, one launch on `stream`; the grid depends on (rows, T, out_stride) only, so
 * the call captures into a hipGraph; one owning thread per output element, no atomics.  A row's result does not depend on rows, on its place
 * in the batch or on out_stride.  Refuses by name before the launch: null pointers, a bad table, track / joints / dir_vec not 16-byte
 * aligned, rows or T < 1, rows not a multiple of draws, frame_unit < 1, an unsupported ratio, a short out_stride, index range. */
int eg_skeleton_joints(const float* track, int32_t rows, int32_t T, const int32_t* parents, const int32_t* children, const float* lengths,
                       int32_t bones, const void* d_table, const int32_t* d_frames, int32_t draws, int32_t frame_unit, const float* d_mean,
                       int32_t unit, int32_t L, int32_t M, float* joints, int64_t out_stride, void* stream);
int eg_skeleton_dir_vec(const float* joints, int32_t rows, int32_t T, const int32_t* parents, const int32_t* children, const float* lengths,
                        int32_t bones, const void* d_table, const int32_t* d_frames, int32_t draws, int32_t frame_unit, const float* d_mean,
                        float* dir_vec, void* stream);

/* Rotations: track [rows, T, 3K] fp32 -> one unit quaternion (w, x, y, z) per bone and output frame, relative to a rest pose: what a rigged
 * avatar (glTF / VRM, a game-engine rig, BVH) consumes.  rotations [rows, out_stride, K, 4] fp32.
 * Inputs.  The bone table as above.  rest [K, 3] float64 on the HOST: the direction of every bone in the avatar's bind pose.  Each row is
 * normalised in float64 (r / sqrt(r . r)) and rounded to fp32; from then on the rows are treated as unit vectors.  A row that is not finite
 * or whose norm is below 1e-6 is refused by name (eg_skeleton_rest_check: host only, no HIP call).
 * Helpers.  pb(k): the bone whose child is parents[k], -1 when parents[k] is the root -- unique (a joint is the child of at most one bone),
 * and pb(k) < k (topological order).  x_k = track[3k .. 3k+2] (+ d_mean) of a source frame; x^_k = x_k / max(|x_k|, 1e-12).
 * arc(a, b) for unit a, b with c = a . b:  c >= -1 + 1e-6: q = (1 + c, a x b) / |(1 + c, a x b)|, the shortest arc, w >= 0;
 * otherwise the half turn q = (0, n), n = (a x e_m) / |a x e_m| with e_m the coordinate axis on which |a| is smallest (the first such axis
 * on ties).  A zero b gives the identity (the formula yields it).
 * Chain, in table order; quaternions are Hamilton products, q o v rotates v by q:
 *     P_k = G_pb(k)                 (the identity when pb(k) = -1)
 *     v_k = conj(P_k) o x^_k        (the bone's direction seen from its parent's frame)
 *     L_k = arc(rest_k, v_k)        (local rotation: a pure swing relative to the parent, w >= 0)
 *     G_k = P_k (x) L_k             (global rotation; its sign is the product's, never flipped)
 * so G_k o rest_k = x^_k for every bone, and forward kinematics with the offsets lengths[k] * rest_k and the locals L_k reproduces
 * eg_skeleton_joints(unit = 1).
 * Frames.  rows, d_frames, draws, frame_unit: "Rows of whole tracks"; the reduced ratio L / M, n_out = ceil(n L / M), lo and f: eg_skeleton_joints.  On
 * an interpolated frame the VECTORS are blended before anything else: x_k = fmaf(x_k(lo + 1) - x_k(lo), f, x_k(lo)), taken after the mean;
 * the chain then runs on the blended frame.  n = 1: frame 0.  At L / M = 1 nothing is blended.
 * Output.  L_k for space = EG_SKELETON_SPACE_LOCAL, G_k for EG_SKELETON_SPACE_GLOBAL.  Frames k' >= n_out are written as zeros; source
 * frames t >= n are never read and may hold NaN.
 * eg_skeleton_levels (host only) writes the device table of the call, EG_SKELETON_LEVEL_WORDS(K) 32-bit words, which the caller uploads as
 * d_levels: [0] the number of depth levels; [1 .. 64] the first position of every level in `order` (the count K from the last level on);
 * order [K]: the bones sorted by depth, table order inside a level; pb [K]; the normalised rest [K, 3] (fp32 bits).  One thread owns one
 * (output frame, bone) and a workgroup walks the levels with one barrier each.  As with d_table nothing ties the upload to the host
 * arguments: with a d_levels that differs the result is unspecified (its numbers are clamped, the accesses stay in range).
 * Guarantees as for eg_skeleton_joints: caller-owned memory, no allocation, no synchronisation, one launch, capturable; one owning thread
 * per output element (each bone's quaternion is one aligned 16-byte store), no atomics; a row's result does not depend on rows, on its
 * place in the batch, on out_stride or on the tile a frame falls in.  Refuses by name before the launch what eg_skeleton_joints refuses,
 * a bad rest row and an unknown space. */
#define EG_SKELETON_SPACE_LOCAL 0
#define EG_SKELETON_SPACE_GLOBAL 1
#define EG_SKELETON_LEVEL_WORDS(K) (65 + 5 * (K))
int eg_skeleton_rest_check(const double* rest, int32_t bones);
int eg_skeleton_levels(const int32_t* parents, const int32_t* children, const float* lengths, int32_t bones, const double* rest,
                       int32_t* words);
int eg_skeleton_rotations(const float* track, int32_t rows, int32_t T, const int32_t* parents, const int32_t* children, const float* lengths,
                          int32_t bones, const double* rest, const void* d_levels, const int32_t* d_frames, int32_t draws, int32_t frame_unit,
                          const float* d_mean, int32_t space, int32_t L, int32_t M, float* rotations, int64_t out_stride, void* stream);

/* Articulated bodies: tracks of 6-D joint rotations (the BEAT generators: pose_dim = 6J) -> joint positions and joint rotations, and back.
 * Body.  J joints in topological order, 1 <= J <= EG_ARTICULATE_MAX_JOINTS: parents[0] = -1, 0 <= parents[j] < j; offsets [J, 3] fp32 in
 * metres, the joint's position in its parent's frame at the bind pose (finite; zero allowed).  eg_articulate_check (host only, no HIP call)
 * refuses by name: J out of range, parents[0] != -1, a parent that is not an earlier joint, an offset that is not finite.
 * 6-D to matrix.  d_j = track[b, t, 6j .. 6j+5] (+ d_mean[6j ..]); a1 = d_j[0..2], a2 = d_j[3..5];
 *     b1 = a1 / max(|a1|, 1e-12);  u2 = a2 - (b1 . a2) b1;  b2 = u2 / max(|u2|, 1e-12);  b3 = b1 x b2.
 * basis = EG_ARTICULATE_BASIS_ROWS: R_j has the rows b1, b2, b3 (pytorch3d's rotation_6d_to_matrix); EG_ARTICULATE_BASIS_COLUMNS: the
 * columns (Zhou et al. 2019).  A degenerate group (zero, or a1 parallel to a2) gives a finite matrix that is not a rotation; every output
 * stays finite.
 * Chain, in table order:  G_0 = R_0, p_0 = offsets[0];  G_j = G_parent R_j,  p_j = p_parent + G_parent offsets[j].
 * Outputs.  joints [rows, out_stride, J, 3] = p.  rotations [rows, out_stride, J, 4]: the unit quaternion (w, x, y, z) of R_j
 * (space = EG_SKELETON_SPACE_LOCAL) or of G_j (EG_SKELETON_SPACE_GLOBAL).  quat(m), with tr = m00 + m11 + m22 and the first largest of
 * (tr, m00, m11, m22):
 *     tr:  (1 + tr, m21 - m12, m02 - m20, m10 - m01)          m00: (m21 - m12, 1 + m00 - m11 - m22, m01 + m10, m02 + m20)
 *     m11: (m02 - m20, m01 + m10, 1 - m00 + m11 - m22, m12 + m21)   m22: (m10 - m01, m02 + m20, m12 + m21, 1 - m00 - m11 + m22)
 * divided by max(|q|, 1e-12) and negated where w < 0, so w >= 0.  Either output pointer may be NULL, not both; one launch writes both.
 * Frames.  rows, d_frames, draws, frame_unit: "Rows of whole tracks"; the reduced ratio L / M, n_out = ceil(n L / M), lo and f: eg_skeleton_joints.  On
 * an interpolated frame the 6-D VECTORS of the source frames lo and lo + 1 are blended, after the mean: d = fmaf(d(lo + 1) - d(lo), f,
 * d(lo)); the whole chain then runs on the blended frame, so the joints and rotations of one call describe the same pose.  n = 1: frame 0.
 * Frames k' >= n_out are written as zeros; source frames t >= n are never read and may hold NaN.
 * eg_articulate_levels (host only) writes the device table of the call, EG_ARTICULATE_LEVEL_WORDS(J) 32-bit words, uploaded by the caller
 * as d_table: [0] the number of depth levels; [1 .. 65] the first position of every level in `order` (J from the last level on);
 * order [J]: the joints sorted by depth, table order inside a level; parents [J]; offsets [J, 3] (fp32 bits).  One thread owns one (output
 * frame, joint of a level) and a workgroup of EG_ARTICULATE_TILE_FRAMES output frames (eg_articulate_tile_frames) walks the levels with one
 * barrier each.  Nothing ties the upload to the host arguments: with a d_table that differs the result is unspecified (its numbers are
 * clamped, the accesses stay in range).
 * Inverse.  eg_articulate_rot6d: quat [rows, T, J, 4] -> rot6d [rows, T, 6J]: q / max(|q|, 1e-12), its matrix, the first two rows (basis
 * rows) or columns (basis columns) as a1 | a2, minus d_mean when given; zeros from frame n on.
 * Guarantees as for eg_skeleton_joints: caller-owned memory, no allocation, no synchronisation, one launch, capturable; one owning thread
 * per output element, no atomics; a row's result does not depend on rows, on its place in the batch or on out_stride.  Refuses by name
 * before the launch: null pointers, a bad body, pointers not 16-byte aligned (d_table / d_mean: 4-byte), rows or T < 1, rows not a
 * multiple of draws, frame_unit < 1, an unknown basis or space, an unsupported ratio, a short out_stride, index range. */
#define EG_ARTICULATE_MAX_JOINTS 64
#define EG_ARTICULATE_TILE_FRAMES 8  /* output frames of one workgroup */
#define EG_ARTICULATE_BASIS_ROWS 0
#define EG_ARTICULATE_BASIS_COLUMNS 1
#define EG_ARTICULATE_LEVEL_WORDS(J) (66 + 5 * (J))
int eg_articulate_check(const int32_t* parents, const float* offsets, int32_t joints);
int eg_articulate_levels(const int32_t* parents, const float* offsets, int32_t joints, int32_t* words);
int32_t eg_articulate_tile_frames(void);
int eg_articulate_forward(const float* track, int32_t rows, int32_t T, const int32_t* parents, const float* offsets, int32_t joints,
                          const void* d_table, const int32_t* d_frames, int32_t draws, int32_t frame_unit, const float* d_mean, int32_t basis,
                          int32_t space, int32_t L, int32_t M, float* out_joints, float* out_rotations, int64_t out_stride, void* stream);
int eg_articulate_rot6d(const float* quat, int32_t rows, int32_t T, int32_t joints, const int32_t* d_frames, int32_t draws,
                        int32_t frame_unit, const float* d_mean, int32_t basis, float* rot6d, void* stream);

/* Euler channels of 6-D rotation tracks (BVH's rotation channels), their inverse, and the Euler filter (csrc/skeleton.hip, csrc/euler.hip).
 * Order.  A joint's channel order is a permutation (i, j, k) of the axes X, Y, Z, as a code: XYZ 0, XZY 1, YXZ 2, YZX 3, ZXY 4, ZYX 5
 * (i = code / 2; the other two ascending for an even code, descending for an odd one).  `Zrotation Xrotation Yrotation` is ZXY and means
 * R = Rz(a) Rx(b) Ry(c) with v_parent = R v_local: the R_j of eg_articulate_forward.  eps = +1 for XYZ, YZX, ZXY and -1 for XZY, YXZ, ZYX.
 * eg_articulate_euler: track [rows, T, 6J] -> euler [rows, out_stride, J, 3].  R_j from the six numbers exactly as in eg_articulate_forward
 * (d_mean, the blend of the 6-D vectors at L / M != 1, Gram-Schmidt, basis), then in fp32 with the library's sqrtf / atan2f:
 *     s = eps R[i][k];   h = sqrt(R[i][i]^2 + R[i][j]^2);   b = atan2(s, h)                       (b in [-pi/2, pi/2])
 *     1 - |s| >= 2^-20:  a = atan2(-eps R[j][k], R[k][k]);  c = atan2(-eps R[i][j], R[i][i])
 *     otherwise (lock):  a = atan2( eps R[k][j], R[j][j]);  c = 0
 * The output holds (a, b, c), the order of the joint's rotation channels, in radians, or with degrees != 0 each times (float)(180 / pi).
 * No tree is involved: one thread per (output frame, joint), no level barriers, a tile of EG_ARTICULATE_TILE_FRAMES output frames per
 * workgroup.  rows, d_frames, draws, frame_unit, L / M, out_stride: as in eg_articulate_forward; frames k' >= n_out are zeros; source
 * frames t >= n are never read and may hold NaN; a degenerate group gives finite angles.  orders: the J codes on the host (checked);
 * d_orders: the same on the device (clamped to 0..5 where they differ).
 * eg_articulate_rot6d_euler: euler [rows, T, J, 3] -> rot6d [rows, T, 6J]: the angles (times (float)(pi / 180) with degrees != 0), the
 * library's sincosf, R = R_i(a) R_j(b) R_k(c) in closed form -- with (sa, sb, sc) the sines times eps and p(.) the place of an axis in the
 * order, R[r][c] = m[p(r)][p(c)] of
 *     m = | cb cc, -cb sc, sb |  | sa sb cc + ca sc, ca cc - sa sb sc, -sa cb |  | sa sc - ca sb cc, sa cc + ca sb sc, ca cb |
 * -- its first two rows (basis rows) or columns as a1 | a2, minus d_mean when given; zeros from frame n on.
 * Both: caller-owned memory, no allocation, no synchronisation, one launch, capturable; one owning thread per output element, no atomics.
 * Refuse by name before the launch: null pointers, joints outside 1 .. EG_ARTICULATE_MAX_JOINTS, an order code outside 0..5, pointers not
 * 16-byte aligned (d_orders / d_mean: 4-byte), rows or T < 1, rows not a multiple of draws, frame_unit < 1, an unknown basis, an
 * unsupported ratio, a short out_stride, grid / index range.
 * eg_angle_unwrap: angles [rows, T, C] fp32, in place; row b has n valid frames as above; every (row, column) is a series p_0 .. p_(n-1):
 *     d_t = p_t - p_(t-1) in fp32;   k_t = nearbyint((double)d_t / period) (ties to even), k_0 = 0;   c_t = k_0 + .. + k_t, a 32-bit integer;
 *     out_t = fmaf(-(float)c_t, (float)period, p_t).
 * Frames t >= n are neither read nor written.  The input is finite and its jumps sum to less than 2^31 periods.  Integer counts make the
 * result independent of the tiling: a tile is EG_UNWRAP_TILE_FRAMES frames; per-tile totals, their scan per row and column, then the
 * pass that writes -- three launches, one when T fits a tile; no atomics.  workspace: eg_angle_unwrap_workspace_bytes bytes
 * of device memory (0 for refused arguments), 4-byte aligned, not read or written when T fits a tile (then it may be NULL).  Capturable.
 * Refuses by name: null angles, rows / T / C < 1, rows not a multiple of draws, frame_unit < 1, a period that is not finite and > 0 in
 * fp32, a missing or short workspace, grid / index range. */
#define EG_UNWRAP_TILE_FRAMES 64
int eg_articulate_euler(const float* track, int32_t rows, int32_t T, int32_t joints, const int32_t* orders, const void* d_orders,
                        const int32_t* d_frames, int32_t draws, int32_t frame_unit, const float* d_mean, int32_t basis, int32_t degrees,
                        int32_t L, int32_t M, float* euler, int64_t out_stride, void* stream);
int eg_articulate_rot6d_euler(const float* euler, int32_t rows, int32_t T, int32_t joints, const int32_t* orders, const void* d_orders,
                              const int32_t* d_frames, int32_t draws, int32_t frame_unit, const float* d_mean, int32_t basis,
                              int32_t degrees, float* rot6d, void* stream);
int64_t eg_angle_unwrap_workspace_bytes(int32_t rows, int32_t T, int32_t C);
int eg_angle_unwrap(float* angles, int32_t rows, int32_t T, int32_t C, const int32_t* d_frames, int32_t draws, int32_t frame_unit,
                    double period, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * BVH text of whole takes: the MOTION lines of every take, formatted on the device (csrc/bvhtext.hip, csrc/bvhtext.h)
 * ------------------------------------------------------------------------------------------ */
/* The text of a finite fp32 v with |v| < 2^31 is "%.6f" of it, defined in integers: q = (double)|v| * 1e6 (exact: 1e6 = 2^6 * 15625, so at
 * most 24 + 14 significant bits, and q < 2^53); N = (uint64) rint(q), ties to even; '-' iff signbit(v) (-0.0 and -1e-9 print "-0.000000", as
 * C does); the decimal digits of N / 10^6 without leading zeros, at least one; '.'; the six digits of N % 10^6.  8 .. EG_BVH_TEXT_MAX_WIDTH
 * bytes.  NaN, an infinity and |v| >= 2^31 are "not writable".
 * eg_bvh_text_decimal (host only, no HIP call, usable without a GPU): the text of v into out (0-terminated) and its length, or -1 for a value
 * that is not writable (or a null out).  It runs the routine the kernels run (csrc/bvhtext.h: egi_decimal6).
 * A take's text.  Row b with n valid frames is n lines; a line is C values joined by one space and ended by '\n'.  Channel c is described
 * by the table, a blob of eg_bvh_text_table_bytes(C) = 28 C bytes: src int32 [C] | const_len int32 [C] | const_text bytes [C][20].
 *     src[c] >= 0          element src[c] of the row's euler [J3] of that frame
 *     src[c] = -1, -2, -3  axis X, Y, Z of root_position [rows / draws, T, 3] (per recording, shared by its draws)
 *     src[c] = -4          the const_len[c] bytes at const_text[c]: text the caller formatted (an OFFSET that need not be an fp32 value)
 * `table` is the blob on the HOST (checked here), d_table the caller's upload of the same bytes; nothing ties the two together: the kernels
 * clamp what they read from d_table, so with an upload that differs the text is unspecified and every access stays in range.
 * Rows: "Rows of whole tracks", with the host copy `frames` and a minimum of 1 valid frame.  The arguments both calls share travel in one
 * block, EgBvhTextArgs.
 * eg_bvh_text_measure: line_off int64 [rows * T + 1]: the byte at which line (b, t) starts, an exclusive scan of the line lengths in
 * (row, frame) order with length 0 for t >= n -- rows are packed back to back, line_off[b * T] is where row b starts and
 * line_off[rows * T] the total.  A value that is not writable counts as "0.000000".  summary (device, 8-byte aligned, 8 + 4 rows bytes): the
 * total (int64), then per row the number of values in its valid frames that are not writable (int32 [rows]).  Three launches -- line
 * lengths and tile totals (a tile is EG_BVH_TEXT_TILE_FRAMES frames of a row), the scan of the totals in one workgroup, the pass that adds
 * a tile's start -- in integers: no atomics, no memset.  workspace: eg_bvh_text_workspace_bytes bytes (0 for refused arguments), 8-byte
 * aligned.
 * eg_bvh_text_write: the text [line_off[rows * T]] bytes into `text` (16-byte aligned), one launch.  A workgroup formats a tile into LDS
 * and streams it out with 16-byte stores over the aligned interior and byte stores for its head and tail.  Values that are not writable
 * are written as "0.000000" (the caller reads summary and refuses them first); no store goes beyond text_bytes or outside the LDS of the
 * workgroup, whatever line_off holds.  Bytes of `text` outside [0, line_off[rows * T]) are not written.
 * Both: caller-owned memory, no allocation, no synchronisation, capturable (grids depend on (rows, T, C) only; C > 431 needs more than 64 KB
 * of LDS, which the first call of a process opts into: make it outside a capture).  A row's bytes do not depend on rows, on its place in
 * the batch or on T.  Refuse by name before the first launch: a null block or null pointers, pointers not aligned as stated, rows or T
 * < 1, C outside 1 .. EG_BVH_TEXT_MAX_CHANNELS, J3 < 1, a src entry outside -4 .. J3 - 1, -1 .. -3 without root_position, a const_len
 * outside 8 .. EG_BVH_TEXT_MAX_WIDTH, rows not a multiple of draws, frame_unit < 1, a host count below 1, a short workspace, text_bytes
 * < 1, grid / index range. */
#define EG_BVH_TEXT_MAX_CHANNELS 512
#define EG_BVH_TEXT_MAX_WIDTH 18
#define EG_BVH_TEXT_TILE_FRAMES 8
typedef struct EgBvhTextArgs {
    const float* euler;          /* device [rows, T, J3] */
    const float* root_position;  /* device [rows / draws, T, 3], or NULL */
    const void* table;           /* host blob */
    const void* d_table;         /* device copy of it */
    const int32_t* frames;       /* host counts [rows / draws], or NULL */
    const int32_t* d_frames;     /* the same on the device */
    int32_t rows, T, J3, C, draws, frame_unit;
} EgBvhTextArgs;
int32_t eg_bvh_text_decimal(float v, char* out);
int32_t eg_bvh_text_tile_frames(void);
int64_t eg_bvh_text_table_bytes(int32_t C);
int64_t eg_bvh_text_workspace_bytes(int32_t rows, int32_t T, int32_t C);
int eg_bvh_text_measure(const EgBvhTextArgs* in, void* workspace, int64_t workspace_bytes, int64_t* line_off, void* summary, void* stream);
int eg_bvh_text_write(const EgBvhTextArgs* in, const int64_t* line_off, void* text, int64_t text_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Preview frames: stick figures of whole takes, one 8-bit picture per frame, drawn on the device (csrc/preview.hip)
 * ------------------------------------------------------------------------------------------ */
/* joints [rows, T, J, 3] fp32 -> out [rows, T, H, W, 3] (layout EG_PREVIEW_HWC) or [rows, T, 3, H, W] (EG_PREVIEW_CHW) uint8.  Rows: "Rows of
 * whole tracks", no minimum: a frame t >= n is all-zero bytes and its joints are never read.
 * Bones.  `bones`: n_bones pairs (ja, jb) of joint indices on the HOST, 1 <= n_bones <= EG_PREVIEW_MAX_BONES, every index in [0, J);
 * eg_preview_check (host only, no HIP call, usable without a GPU) refuses anything else by name.  d_table, the device copy, is
 * EG_PREVIEW_TABLE_WORDS 32-bit words, 16-byte aligned:
 *     [0] n_bones | [1] n_used | [2] background (r | g << 8 | b << 16) | [3] 0 | used [128]: the distinct joints the bones name, ascending |
 *     a [64], b [64]: the two ends of bone k as positions in `used` | colour [64] (packed as the background)
 * Nothing ties the upload to the host list: the kernel clamps what it reads from d_table, so with an upload that differs the picture is
 * unspecified and every access stays in range.  The three channels are bytes to the device, whatever colour space the caller means.
 * Camera.  `camera`: 8 fp32 on the HOST, read at the call and passed by value -- M00 M01 M02 M10 M11 M12 c0 c1.
 * One frame.  Every + - x below is one IEEE fp32 operation in the order written (no fused multiply-add); the square root and the reciprocal
 * are correctly rounded; a comparison with a NaN is false.
 *     u_j = ((M00 x_j + M01 y_j) + M02 z_j) + c0,   v_j = ((M10 x_j + M11 y_j) + M12 z_j) + c1         per joint the bones name
 *     picture = background;  per bone k = (ja, jb), in the order of `bones`:
 *         ax, ay = u_ja, v_ja;  ex = u_jb - ax;  ey = v_jb - ay;  l2 = ex ex + ey ey;  inv = l2 > 0 ? 1 / l2 : 0
 *         per pixel (px, py), X = px + 0.5, Y = py + 0.5:
 *             wx = X - ax;  wy = Y - ay;  s = (wx ex + wy ey) inv;  t = s < 0 ? 0 : s;  t = t > 1 ? 1 : t          (a NaN stays a NaN)
 *             dx = wx - t ex;  dy = wy - t ey;  a = (radius + 0.5) - sqrt(dx dx + dy dy)
 *             q = a >= 1 ? 255 : a > 0 ? (int)(a 255 + 0.5) : 0                                                     (a NaN: q = 0)
 *             every channel:  c = (c (255 - q) + colour[k] q + 127) / 255                                          in integers
 * Later bones paint over earlier ones; a bone of zero length is a disc; a bone with an end that is not finite draws nothing (every q is 0).
 * eg_preview_raster: one launch on `stream`, one workgroup per (frame, band of image rows).  The frame's projected joints and bone
 * parameters are made once per workgroup in LDS, and the workgroup keeps the list of the bones whose bounding box -- grown by radius + 1
 * and by 2^-20 of the largest coordinate, more than the rounding of the formula can move a pixel's distance -- touches its rows; a wave
 * composites a block of the band in LDS, walking only the boxes of the listed bones, and every thread then stores 16 consecutive pixels of
 * a row with 16-byte stores (W not a multiple of 16: the same bytes through stores that assume no alignment, and a narrower tail).  The
 * picture is that of the formula, not of the boxes.  No allocation, no synchronisation, no atomics, no
 * memset; the grid depends on (rows, T, H, W) only, so the call captures into a hipGraph.  A row's pictures do not depend on rows, on its
 * place in the batch or on T.  Refuses by name before the launch: null pointers, joints / out / d_table not 16-byte aligned, rows, T or J < 1,
 * a bad bones list (as eg_preview_check), H or W outside EG_PREVIEW_MIN_SIZE .. EG_PREVIEW_MAX_SIZE, a radius outside
 * EG_PREVIEW_MIN_RADIUS .. EG_PREVIEW_MAX_RADIUS (or NaN), a camera entry that is not finite, an unknown layout, rows not a multiple of draws,
 * frame_unit < 1, d_frames not 4-byte aligned, grid / index range.
 * eg_preview_max_bones: EG_PREVIEW_MAX_BONES. */
#define EG_PREVIEW_MAX_BONES 64
#define EG_PREVIEW_MIN_SIZE 8
#define EG_PREVIEW_MAX_SIZE 2048
#define EG_PREVIEW_MIN_RADIUS 0.25f
#define EG_PREVIEW_MAX_RADIUS 16.0f
#define EG_PREVIEW_TABLE_WORDS 324  /* 4 + 2 * EG_PREVIEW_MAX_BONES + 3 * EG_PREVIEW_MAX_BONES */
#define EG_PREVIEW_HWC 0
#define EG_PREVIEW_CHW 1
int32_t eg_preview_max_bones(void);
int eg_preview_check(const int32_t* bones, int32_t n_bones, int32_t J);
int eg_preview_raster(const float* joints, int32_t rows, int32_t T, int32_t J, const int32_t* bones, int32_t n_bones, const int32_t* d_table,
                      const float* camera, float radius, int32_t H, int32_t W, int32_t layout, int32_t draws, int32_t frame_unit,
                      const int32_t* d_frames, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Smoothed output: a Savitzky-Golay filter along the time axis of whole tracks on the device (csrc/smooth.hip)
 * ------------------------------------------------------------------------------------------ */
/* A filter is (window K, polyorder p, deriv d, delta): K odd, 3 <= K <= EG_SMOOTH_MAX_WINDOW; 1 <= p <= min(5, K - 1); 0 <= d <= min(2, p);
 * delta = 1 / fps > 0 (it matters for d > 0 only); half = K / 2.
 * eg_smooth_design (host only, no HIP call, usable without a GPU; refuses a bad K, p, d or delta by name) writes the table C[K][K]: row i
 * holds the weights that give the d-th derivative at window position i of the least-squares polynomial of degree p through K equally spaced
 * samples.  Designed in float64 with the abscissae centred on the window (t = j - half) and a QR factorisation; table32 is table64 rounded
 * once to fp32 and is what the device reads (either pointer may be NULL, not both).
 * Definition.  For a row with n >= K valid frames and every column:
 *     head      i < half:             y[i] = sum_j C[i][j] x[j]
 *     interior  half <= i < n - half: y[i] = sum_j C[half][j] x[i - half + j]
 *     tail      i >= n - half:        y[i] = sum_j C[K - (n - i)][j] x[n - K + j]
 * which is scipy.signal.savgol_filter(x, K, p, deriv=d, delta=delta, axis=0, mode="interp").  Frames i >= n of the output are zeros; source
 * frames t >= n are never read and may hold NaN; no sample outside [0, n) enters any output (no padding at the ends).  On the device every
 * output element is acc = 0, then acc = fmaf(C[.][j], x[.], acc) for j = 0 .. K - 1 in that order, in fp32.
 * eg_smooth_tracks: track [rows, T, D] fp32 -> out [rows, T, D] fp32.  Row b has n valid frames and the call takes
 * the host copy `frames` ("Rows of whole tracks"): a row with n < K is refused by name -- there is no shrinking window --, and a row
 * whose device count is below K although the host count is not comes out as zeros.  d_table: device copy of table32.
 * All pointers are caller-owned; no allocation, no synchronisation, one launch on `stream`; the grid -- (tile of EG_SMOOTH_TILE_FRAMES
 * frames) x (tile of EG_SMOOTH_TILE_COLS columns) x row -- depends on (rows, T, D) only, so the call captures into a hipGraph; one owning
 * thread per output element, plain vector stores, no atomics.  A row's result does not depend on rows, on its place in the batch or on T.
 * Refuses by name before the launch: null pointers, track / out / d_table not 16-byte aligned, out overlapping track, rows, T or D < 1, rows
 * not a multiple of draws, frame_unit < 1, K out of range or even, a count below K, grid / index range.
 * eg_smooth_tile_frames / eg_smooth_tile_cols: the two tile sizes. */
#define EG_SMOOTH_MAX_WINDOW 31
#define EG_SMOOTH_TILE_FRAMES 64
#define EG_SMOOTH_TILE_COLS 64
int eg_smooth_design(int32_t K, int32_t p, int32_t d, double delta, double* table64, float* table32);
int32_t eg_smooth_tile_frames(void);
int32_t eg_smooth_tile_cols(void);
int eg_smooth_tracks(const float* track, int32_t rows, int32_t T, int32_t D, int32_t K, const float* d_table, const int32_t* frames,
                     const int32_t* d_frames, int32_t draws, int32_t frame_unit, float* out, void* stream);
/* Stream: the same filter on a track that arrives H frames per step.  state = the last K - 1 raw frames [rows, K - 1, D] fp32 followed by
 * an int32 count of valid steps per row, in a caller-owned device buffer of eg_smooth_stream_state_bytes (0 for refused arguments).
 * eg_smooth_stream_reset zeroes history and count of the rows with row_mask[u] != 0 (device int32 [rows]; NULL: every row).
 * eg_smooth_stream_push: chunk [rows, H, D], the raw rows the step just emitted, and d_valid (device int32 [rows], the step's valid flags;
 * NULL: every row) -> out [rows, H, D].  A valid row in its s-th valid step gets the smoothed frames [sH - half, (s + 1)H - half) of its
 * track -- the output runs `half` frames behind the input; entries with a negative frame index, the first `half` of step 0, are zeros.  A
 * row that is not valid gets zeros and its state stays as it is.  K <= H is required (the head frames need x[0 .. K) inside the first
 * chunk).  Two launches: the outputs, then the new history and count in a launch of their own, so no launch reads and overwrites the state.
 * eg_smooth_stream_tail: tail_rows [rows, P, D], the last P raw frames of every track (eg_stream_tail's; P >= 1) -> out [rows, P + half, D],
 * the last P + half smoothed frames (zeros for a row without a valid step); the state is read only.
 * Every element comes from the device function the offline kernel uses: the pushes of a row, concatenated after dropping step 0's `half`
 * leading zeros, followed by the tail, are eg_smooth_tracks on the finished track bit for bit. */
int64_t eg_smooth_stream_state_bytes(int32_t rows, int32_t D, int32_t K);
int eg_smooth_stream_reset(void* state, int32_t rows, int32_t D, int32_t K, const int32_t* row_mask, void* stream);
int eg_smooth_stream_push(void* state, int32_t rows, int32_t H, int32_t D, int32_t K, const float* d_table, const float* chunk,
                          const int32_t* d_valid, float* out, void* stream);
int eg_smooth_stream_tail(const void* state, int32_t rows, int32_t P, int32_t D, int32_t K, const float* d_table, const float* tail_rows,
                          float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Delayed output stage of a stream: smoothed joints, rotations and Euler channels at a renderer's frame rate (csrc/render_stream.hip,
 * csrc/skeleton.hip)
 * ------------------------------------------------------------------------------------------ */
/* A stream emits H pose frames per step.  The Savitzky-Golay filter needs `half` frames behind a frame, the interpolator of a frame-rate
 * change (L / M reduced, eg_skeleton_joints) the source frame after it.  Let the output run d source frames behind the rows just emitted:
 *     d0 = half + (L == M ? 0 : 1);   d = M ceil(d0 / M);   delta = d - half;   Hout = H L / M;   lead = d L / M
 * (H a multiple of M, d <= H; the caller's to check).  With y the smoothed track (eg_smooth_stream_push's output, which starts at frame
 * sH - half in a row's s-th valid step; or the raw track with half = 0), that step's outputs are the first Hout output frames of the
 * window y[sH - d .. sH - d + W), W = H + (L != M), run as a row of its own: d L / M and H L / M are integers, so the window starts at phase 0
 * and its output frame j is output frame (sH - d) L / M + j of the whole track -- the same lo, the same weight (k' M - lo L) / L in integers,
 * the same arithmetic, and the clamp lo <= n - 2 is never reached: the same bits.  Frames before frame 0 do not exist: the first `lead`
 * outputs of a row's first valid step are zeros.
 * Delay line.  state: the last delta frames of y [rows, delta, D] fp32, then an int32 count of valid steps per row, in a caller-owned
 * device buffer of eg_render_stream_state_bytes (0 for refused arguments), 16-byte aligned.  0 <= delta <= EG_RENDER_STREAM_MAX_DELTA.
 * eg_render_stream_reset zeroes history and count of the rows with row_mask[u] != 0 (device int32 [rows]; NULL: every row).
 * eg_render_stream_push: chunk [rows, H, D] and d_valid (device int32 [rows]; NULL: every row) -> window [rows, frames, D] =
 * history | chunk[0 .. frames - delta) for the valid rows (delta < frames <= delta + H; the window of a row that is not valid is not
 * written and never read), and d_window, device int32 [2, rows]: the valid frames of every row's window (frames, or 0) | its zeroed head
 * (lead in a row's first valid step, else 0).  Then, in a launch of their own, the new history -- the chunk's last delta frames -- and
 * the count, for the valid rows; the state of a row that is not valid stays.  Two launches, nothing that depends on the step index.
 * eg_render_stream_tail: last [rows, F, D], the last F frames of y (eg_smooth_stream_tail's P + half, or eg_stream_tail's P) ->
 * window [rows, delta + F, D] = history | last and d_window = (delta + F, or 0 for a row without a valid step) | 0: the window
 * y[SH - d .. T) of a track of S steps, whose outputs as an ordinary row of delta + F frames are the track's last ceil((d + P) L / M)
 * output frames, its extrapolated last frames included (the clamp falls on the same frame).  One launch; the state is read only.
 * One owning thread per element, 16-byte stores where a quad lies inside a row, no atomics, no memset.
 * Window form of the forward kernels.  eg_skeleton_joints_window, eg_skeleton_rotations_window, eg_articulate_forward_window and
 * eg_articulate_euler_window are eg_skeleton_joints, eg_skeleton_rotations, eg_articulate_forward and eg_articulate_euler on
 * window [rows, T, .] with draws = frame_unit = 1 and two differences: the output has out_frames frames per row, 1 <= out_frames <=
 * ceil(T L / M) -- frames from there on are not made --, and d_window (device int32 [2, rows], required) gives every row's valid source
 * frames n and, behind them, the number of its leading output frames that are written as zeros.  Every other output frame has the bits
 * of the whole-track call on the same row.  They are separate instantiations of the same kernels; the whole-track calls are unchanged. */
#define EG_RENDER_STREAM_MAX_DELTA 64
int64_t eg_render_stream_state_bytes(int32_t rows, int32_t D, int32_t delta);
int eg_render_stream_reset(void* state, int32_t rows, int32_t D, int32_t delta, const int32_t* row_mask, void* stream);
int eg_render_stream_push(void* state, int32_t rows, int32_t H, int32_t D, int32_t delta, int32_t frames, int32_t lead, const float* chunk,
                          const int32_t* d_valid, float* window, int32_t* d_window, void* stream);
int eg_render_stream_tail(const void* state, int32_t rows, int32_t F, int32_t D, int32_t delta, const float* last, float* window,
                          int32_t* d_window, void* stream);
int eg_skeleton_joints_window(const float* window, int32_t rows, int32_t T, const int32_t* parents, const int32_t* children,
                              const float* lengths, int32_t bones, const void* d_table, const int32_t* d_window, const float* d_mean,
                              int32_t unit, int32_t L, int32_t M, float* joints, int64_t out_frames, void* stream);
int eg_skeleton_rotations_window(const float* window, int32_t rows, int32_t T, const int32_t* parents, const int32_t* children,
                                 const float* lengths, int32_t bones, const double* rest, const void* d_levels, const int32_t* d_window,
                                 const float* d_mean, int32_t space, int32_t L, int32_t M, float* rotations, int64_t out_frames, void* stream);
int eg_articulate_forward_window(const float* window, int32_t rows, int32_t T, const int32_t* parents, const float* offsets, int32_t joints,
                                 const void* d_table, const int32_t* d_window, const float* d_mean, int32_t basis, int32_t space, int32_t L,
                                 int32_t M, float* out_joints, float* out_rotations, int64_t out_frames, void* stream);
int eg_articulate_euler_window(const float* window, int32_t rows, int32_t T, int32_t joints, const int32_t* orders, const void* d_orders,
                               const int32_t* d_window, const float* d_mean, int32_t basis, int32_t degrees, int32_t L, int32_t M, float* euler,
                               int64_t out_frames, void* stream);

/* ------------------------------------------------------------------------------------------
 * Motion statistics of whole tracks: mean speed, acceleration and jerk per joint and a histogram of the joint speeds (csrc/kinematics.hip)
 * ------------------------------------------------------------------------------------------ */
/* Input: joint positions p [rows, T, J, 3] in fp32 metres (what eg_skeleton_joints / eg_articulate_forward write).  Row b has
 * n valid frames ("Rows of whole tracks"); frames t >= n may hold
 * NaN and no sample at or beyond n enters any output.
 * Differences, in fp32, one IEEE subtraction each, by successive differencing:
 *     d1[t] = p[t+1] - p[t] for t < n - 1;   d2[t] = d1[t+1] - d1[t] for t < n - 2;   d3[t] = d2[t+1] - d2[t] for t < n - 3
 * (no product in these steps, so contraction cannot change them and numpy in float32 reproduces them bit for bit).
 * Squared magnitudes: s2_k[t, j] = (x*x + y*y) + z*z in fp64 of the three fp32 components of d_k[t, j], widened first: every square is exact
 * (24-bit operands), so the value is the same with or without fused multiply-add.
 * Means: mean[b, k - 1, j] = (sum_t sqrt(s2_k[t, j])) * fps^k / (n - k) for k = 1, 2, 3 -- m/s, m/s^2, m/s^3 --, the sum in fp64 in a fixed
 * order that depends on the row's own n and on EG_KIN_TILE_FRAMES only; fps, fps^2 and fps^3 are formed on the host in fp64.
 * Speed histogram: `edges` are E = bins + 1 ascending fp64 values in m/s with edges[0] == 0.  eg_kin_edges2 (host only, no HIP call, usable
 * without a GPU) writes edges2[e] = q * q with q = edges[e] / fps, two fp64 operations; it refuses by name fewer than 2 or more than
 * EG_KIN_MAX_BINS + 1 edges, edges[0] != 0, edges that are not strictly ascending, non-finite values and an fps that is not finite and > 0.
 * Speed sample (t, j) falls into bin e when edges2[e] <= s2_1 < edges2[e + 1] and into the overflow column `bins` when s2_1 >= edges2[bins]
 * (a value exactly on an edge belongs to the upper bin; no square root and no division for binning).  hist [rows, J, bins + 1] int32, the
 * last column the overflow; hist[b, j] sums to n - 1.
 * eg_kin_stats: three launches on `stream` -- hist = 0, the tiles, the means --; no allocation, no synchronisation, no floating-point
 * atomics (integer atomics for the bins: order-free), plain vector stores; the grids depend on (rows, T, J, bins) only, so the call captures
 * into a hipGraph.  A row's result does not depend on rows, on its place in the batch or on T.  workspace: eg_kin_workspace_bytes (0 for
 * refused arguments), the [rows, tiles, 3, J] fp64 tile sums.  d_edges2: device copy of eg_kin_edges2's table.
 * A row with n < 4 is refused by name from `frames`, the host copy of the counts ("Rows of whole tracks"); with a device count below 4 although the host count is not, that row's outputs are zeros and every
 * access stays in range.
 * Refuses by name before the first launch: null pointers, joints / workspace / mean / hist not 16-byte aligned, rows < 1, T < 4, J outside
 * 1..EG_KIN_MAX_JOINTS, bins outside 1..EG_KIN_MAX_BINS, rows not a multiple of draws, frame_unit < 1, fps not finite or not positive, a host
 * count below 4, a short workspace, grid / index range. */
#define EG_KIN_MAX_JOINTS 64
#define EG_KIN_MAX_BINS 256
#define EG_KIN_TILE_FRAMES 64
int32_t eg_kin_tile_frames(void);
int eg_kin_edges2(const double* edges, int32_t n_edges, double fps, double* edges2);
int64_t eg_kin_workspace_bytes(int32_t rows, int32_t T, int32_t J, int32_t bins);
int eg_kin_stats(const float* joints, int32_t rows, int32_t T, int32_t J, const int32_t* frames, const int32_t* d_frames, int32_t draws,
                 int32_t frame_unit, double fps, const double* d_edges2, int32_t bins, void* workspace, int64_t workspace_bytes, double* mean,
                 int32_t* hist, void* stream);

/* ------------------------------------------------------------------------------------------
 * Joint-space scores of whole tracks: SRGR (semantic-relevant gesture recall) and L1 diversity, model/Beat_score_v2.py SRGR / L1div
 * (csrc/jointscore.hip)
 * ------------------------------------------------------------------------------------------ */
/* Rows: "Rows of whole tracks", with the host copy `frames` and a minimum of 1 valid frame.  A row's result depends on its own data and n
 * only -- not on rows, on its place in the batch or on T.
 *
 * SRGR.  results r [rows, T, J, 3] fp32; targets g [rows / draws, T, J, 3] fp32, one per recording, shared by its `draws` takes; semantic
 * weights w [rows / draws, T] fp32 (NULL: every weight 1); threshold and scale fp64 (the reference's normaliser is scale = 1 / 0.165, formed
 * on the host).
 *     d[t, j] = (|rx - gx| + |ry - gy|) + |rz - gz|    each difference one IEEE fp32 subtraction, the absolute values widened to fp64, the two
 *                                                      fp64 additions in that order (no product: nothing to contract)
 *     hit[t, j] = d[t, j] < threshold                  a value equal to the threshold is a miss, and so is a NaN
 *     hits[b, j] = sum_t hit[t, j]                     int32, exact
 *     c[t] = sum_j hit[t, j];   weighted[b] = sum_t double(w[t]) * c[t]     every product exact (24 x 7 bits); the sum in fp64: the frames of a
 *                                                      tile of EG_JOINTSCORE_TILE_FRAMES in ascending order from 0, then the row's tiles in
 *                                                      ascending order -- an order that depends on n and the tile size only
 *     srgr[b] = weighted[b] * scale / (n * J);   recall[b] = (sum_j hits[b, j]) / (n * J)         fp64
 * Error of srgr against the exact sum: the first-order bound of a fixed-order fp64 sum of n terms, (n + 8) * 2^-53 * sum_t |w[t]| c[t] *
 * scale / (n J) (the scale, the division and the reference sum's own rounding are the 8).
 * eg_srgr_tracks: two launches on `stream` -- the tiles, the finalise --; no allocation, no synchronisation, no memset and no atomics: a
 * workgroup owns one tile of one row and stores its partials (one fp64 and J int32) to the workspace, and the finalise adds a row's own
 * ceil(n / tile) tiles.  The grids depend on (rows, T, J, draws) only, so the call captures into a hipGraph; the takes of a recording are
 * neighbours in the grid (they read one target tile).  workspace: eg_srgr_workspace_bytes (0 for refused arguments).
 *
 * L1 diversity.  x [rows, T, D] fp32, any column layout (joints as J*3 columns, a 126- or 282-column track, Euler channels), never written.
 *     mean[b, c] = (sum_t double(x[t, c])) / n;   l1_sum[b] = sum_t sum_c |double(x[t, c]) - mean[b, c]|;   l1div[b] = l1_sum[b] / n
 * Both sums in fp64 in a fixed order that depends on n, D and the kernel's tile constants only (runs of frames of a tile ascending, the runs
 * of a tile ascending, the columns by a fixed tree, the tiles ascending).  Against the exact values (S = sum |x - m|, A = sum |x| over the
 * row, m the exact mean): |mean - m| <= (n + 8) * 2^-53 * sum_t |x[t, c]| / n per column, and
 *     |l1_sum - S| <= 2^-53 * ((n D + 8) * S + 2 (n + 8) * A)
 * -- the first-order bound of any fixed summation order of n D terms plus the mean's error carried through n frames.
 * eg_l1div_tracks: four launches on `stream` -- column sums, means, deviations, finalise --; otherwise as eg_srgr_tracks.  workspace:
 * eg_l1div_workspace_bytes, the [rows, tiles, D] and [rows, tiles] fp64 tile sums.
 *
 * Both refuse by name before the first launch: null pointers (semantic may be NULL), results / targets / x / workspace not 16-byte aligned,
 * fp64 outputs not 8-byte and int32 arrays not 4-byte aligned, rows < 1, T < 1, J outside 1..EG_SRGR_MAX_JOINTS, D outside
 * 1..EG_L1DIV_MAX_COLS, rows not a multiple of draws, frame_unit < 1, a threshold or scale that is not finite, a host count below 1, a
 * short workspace, grid / index range. */
#define EG_JOINTSCORE_TILE_FRAMES 32
#define EG_SRGR_MAX_JOINTS 64
#define EG_L1DIV_MAX_COLS 512
int32_t eg_jointscore_tile_frames(void);
int64_t eg_srgr_workspace_bytes(int32_t rows, int32_t T, int32_t J);
int eg_srgr_tracks(const float* results, const float* targets, const float* semantic, int32_t rows, int32_t T, int32_t J,
                   const int32_t* frames, const int32_t* d_frames, int32_t draws, int32_t frame_unit, double threshold, double scale,
                   void* workspace, int64_t workspace_bytes, double* srgr, double* recall, int32_t* hits, void* stream);
int64_t eg_l1div_workspace_bytes(int32_t rows, int32_t T, int32_t D);
int eg_l1div_tracks(const float* x, int32_t rows, int32_t T, int32_t D, const int32_t* frames, const int32_t* d_frames, int32_t draws,
                    int32_t frame_unit, void* workspace, int64_t workspace_bytes, double* mean, double* l1_sum, double* l1div, void* stream);

/* ------------------------------------------------------------------------------------------
 * Beat-alignment score = model/Beat_score_v2.py alignment(sigma, order): load_audio + load_pose +
 * calculate_align for a batch of clips (test_emotion_gesture_diversity_iterative.py:241-248)
 * ------------------------------------------------------------------------------------------ */
/* The audio half restates librosa 0.10's onset_strength / onset_detect / onset_backtrack / feature.rms (n_fft 2048, hop 512, centred,
 * zero pad, 128 Slaney mels, power_to_db(ref=1.0, top_db=80), peak picking with librosa's default sr 22050); it is not pinned against
 * librosa itself.
 * audio [B, n_samples] fp32 16 kHz, already starting at t_start (the caller slices); T = 1 + n_samples/512 onset frames,
 * n_samples >= 2048 and T <= EG_BEAT_MAX_FRAMES (n_samples < 524288: 32 s; a BEAT 10 s clip has T = 313).
 * pose [B, frames, pose_dim] fp32 (pose_dim >= 174: the beat joints are columns 18:42 and 150:174), frames - 1 <= EG_BEAT_MAX_FRAMES;
 * the right-side curves are sliced [t_start*pose_fps : t_end*pose_fps] as upstream; sigma > 0, order >= 1, 0 <= t_start < t_end.
 * pose == NULL: audio half only (score and pose_beats unused).
 * Outputs, each written only when non-NULL (score required with a pose):
 *   score [B] fp64 (NaN for a clip without audio onsets), n_audio_beats [B] (onset_raw count), oenv / rms [B, T],
 *   audio_beats [B, 3, T] uint8 (onset_raw 0/1; onset_bt, onset_bt_rms as multiplicities: two onsets can backtrack to one frame),
 *   pose_beats [B, 8, frames-1] uint8 in load_pose's return order (right arm, shoulder, fore arm, wrist, left ...; the right-side
 *   indices are relative to the slice start, as upstream).
 * d_melfb_t [1025,128], d_window [2048], d_twiddle [1024,2], d_band [128,2]: device copies of eg_beat_tables.
 * workspace >= eg_beat_workspace_bytes.  Deterministic (fixed summation orders), stream-ordered, no host synchronisation. */
#define EG_BEAT_MAX_FRAMES 1024
int eg_beat_tables(float* h_melfb_t /*1025*128, transposed*/, float* h_window /*2048*/, float* h_twiddle /*2*1024*/,
                   int32_t* h_band /*128*2*/);
int64_t eg_beat_workspace_bytes(int32_t batch, int32_t n_samples);
int eg_beat_align(const float* audio, int32_t batch, int32_t n_samples, const float* pose, int32_t frames, int32_t pose_dim,
                  int32_t pose_fps, int32_t t_start, int32_t t_end, double sigma, int32_t order, const float* d_melfb_t,
                  const float* d_window, const float* d_twiddle, const int32_t* d_band, void* workspace, int64_t workspace_bytes,
                  double* score, int32_t* n_audio_beats, float* oenv, float* rms, uint8_t* audio_beats, uint8_t* pose_beats,
                  void* stream);

/* The same score for whole recordings of any and unequal length, R gesture tracks ("draws") per recording: the score of a synthesize()
 * roll-out.  EG_BEAT_MAX_FRAMES does not apply: the per-frame arrays live in the workspace, packed recording after recording, and every
 * stage that grows with the recording is a grid over the chip (csrc/beat_tracks.hip).  The audio half of a recording is computed once and
 * serves all its draws.  A recording that fits eg_beat_align gets, for every output, the bits eg_beat_align gives on its trimmed rows.
 *
 * audio [U, stride] fp32 16 kHz, row u holds lengths[u] real samples (already sliced at t_start * 16000); nothing past lengths[u] is read.
 * pose [U, draws, Tmax, pose_dim] fp32, recording u has frames[u] real poses; pose == NULL: audio half only (draws / Tmax / frames / score /
 * pose_beats unused).  lengths / frames / t_end: HOST arrays [U]; t_end == NULL: frames[u] / pose_fps per recording.
 *
 * d_meta: a device copy of the table eg_beat_tracks_meta writes (eg_beat_tracks_meta_ints(U) int32: a head {U, sum T, max T, max frames}, then
 * per recording {length, T_u = 1 + length / 512, frames, offset = sum of the earlier T, t_end, 0, 0, 0}); host only, no HIP call.  The caller
 * uploads it once per (lengths, frames, t_end) and passes the same host vectors to the call, which checks them but does not read d_meta.
 *
 * Outputs, each written only when non-NULL (score required with a pose): score [U * draws] fp64 (NaN for a recording without onsets),
 * n_audio_beats [U], oenv / rms [sum T] packed at the table's offsets, audio_beats [3, sum T] uint8 (as eg_beat_align's, packed),
 * pose_beats [U * draws, 8, Tmax - 1] uint8 (zero past a recording's own frames).
 * Refused with the argument's name: null required pointers, U < 1, draws < 1, lengths[u] < 2048 or > stride, frames[u] < 2 or > Tmax,
 * pose_dim < 174, pose_fps <= 0, order < 1, sigma <= 0, t_start < 0, t_end[u] <= t_start, a workspace below eg_beat_tracks_workspace_bytes
 * (which is 0 for a refused shape), and sizes beyond the index types: sum T > 2^24, U or U * draws > 65535, U * draws * 8 * (Tmax - 1) >= 2^31.
 * One hour per recording (T = 112501, 54000 poses) is well inside.  Deterministic, stream-ordered, no allocation, no host synchronisation;
 * launches, grids and pointers depend on (lengths, frames, draws) only, so the call captures into a hipGraph. */
int64_t eg_beat_tracks_meta_ints(int32_t recordings);
int eg_beat_tracks_meta(const int32_t* lengths, const int32_t* frames /*NULL: audio only*/, const int32_t* t_end /*NULL: frames/fps*/,
                        int32_t pose_fps, int32_t recordings, int32_t* meta);
int64_t eg_beat_tracks_workspace_bytes(const int32_t* lengths, const int32_t* frames /*NULL: audio only*/, int32_t recordings, int32_t draws,
                                       int32_t Tmax);
int eg_beat_align_tracks(const float* audio, int32_t recordings, int64_t stride, const int32_t* lengths, const int32_t* d_meta,
                         const float* pose, int32_t draws, int32_t Tmax, int32_t pose_dim, const int32_t* frames, int32_t pose_fps,
                         int32_t t_start, const int32_t* t_end, double sigma, int32_t order, const float* d_melfb_t, const float* d_window,
                         const float* d_twiddle, const int32_t* d_band, void* workspace, int64_t workspace_bytes, double* score,
                         int32_t* n_audio_beats, float* oenv, float* rms, uint8_t* audio_beats, uint8_t* pose_beats, void* stream);
/* Test entry: the wait-suppressed scan of peak_pick as the per-frame rule "accepted iff a candidate at an even offset from the start of its
 * run of candidates" plus the compaction, on a caller-made d_cand [sum T] uint8 packed as the table places the recordings.  events [sum T]
 * int32 (recording u's accepted frames ascending from its offset), counts [U]; workspace as for the audio half. */
int eg_beat_tracks_scan(const uint8_t* d_cand, const int32_t* lengths, int32_t recordings, const int32_t* d_meta, void* workspace,
                        int64_t workspace_bytes, int32_t* events, int32_t* counts, void* stream);

/* Take diversity of whole tracks: the FGD features of a synthesize() roll-out and the pairwise distances of the R takes ("draws") of one
 * recording (csrc/takes.hip) -- the whole-track counterpart of eg_beat_align_tracks for the FGD / Div_score half of the eval loop's summary
 * line (test_emotion_gesture_diversity_iterative.py:250-261).  The FGD encoder itself (model/FGD.py:26-82) is three eg_linear products on
 * the packed rows; these entries are everything around it.
 *
 * Inputs.  track [U, R, Tmax, D] fp32 on the device; frames[u] in 1 .. Tmax on the HOST, the real poses of recording u.  Rows at or beyond
 * frames[u] are never read: they may hold anything, NaN included.
 * Packed order: recording-major, then draw, then frame.  With off[u] the exclusive prefix sum of frames, row R*off[u] + r*frames[u] + t
 * holds pose (u, r, t); the row count is N = R * sum(frames).
 * Meta table (host only: no HIP call, usable without a GPU): eg_take_meta writes `frames | off`, 2U int32 (the count eg_take_meta_ints
 * returns; 0 for U < 1 or U > 65535).  The caller uploads it once per frames vector and passes the device copy as d_meta beside the host
 * vector; the kernels read d_meta, the host checks `frames`.  Refuses by name: null pointers, U outside 1 .. 65535, frames[u] < 1,
 * sum(frames) >= 2^31.
 *
 * eg_track_rows_pack: rows [N, Dpad], Dpad = 4*ceil(D/4): the valid rows of `track` in packed order, the pad columns written as zeros --
 * the K % 4 == 0 input eg_linear wants, without a concatenation per call.  One launch gridded over the chip; every output element has one
 * owning thread; 16-byte stores, 16-byte loads where D % 4 == 0 and `track` is 16-byte aligned, scalar loads otherwise (D = 282 and 126).
 * draws >= 1 here.  Refuses by name: null pointers, rows not 16-byte aligned, U outside 1 .. 65535, draws outside 1 .. EG_TAKE_MAX_DRAWS,
 * Tmax < 1, D < 1, frames[u] outside 1 .. Tmax, N * Dpad >= 2^40.
 *
 * eg_take_distance on packed features feat [N, K] fp32 (K = 512 for the FGD encoder; any multiple of 4):
 *   S[u, r, r']        = sum_{t < frames[u]} sum_{k < K} (feat[u,r,t,k] - feat[u,r',t,k])^2
 *   distance[u, r, r'] = sqrt(S * scale_u),  scale_u = 1 when span <= 0 ("None": exactly the pair distance of model/FHD_score.py:270-286 on
 *                        activations of frames[u] rows), scale_u = span / frames[u] otherwise: the same quantity brought to the scale of
 *                        a span-frame clip, so takes of a 30 s and of a 60 s recording, and the clip metric at frames == span, read in one unit
 *   diversity[u]       = 2 / (R (R - 1)) * sum_{r < r'} distance[u, r, r'], summed in lexicographic pair order
 * Differences, squares and sums are fp64, each fp32 operand widened before the subtraction.  distance [U, R, R] fp64 is symmetric bit for
 * bit with an exactly zero diagonal; diversity [U] fp64.
 * Stage 1: the frames of every recording are cut into chunks of EG_TAKE_CHUNK_FRAMES frames (the result may depend on that constant and
 * on nothing else: not on U, not on the recording's place in the batch, not on the order of the draws); grid over (chunk, base take r).
 * A workgroup keeps take r's chunk in registers while looping r' > r (the re-reads of the other takes' chunks are served by L2), reduces
 * lane -> wave -> workgroup in a fixed order and one thread per pair stores the partial to workspace[chunk, pair] -- no floating-point
 * atomics.  Stage 2 (second launch): per (u, pair) the chunk partials summed in ascending chunk order, scale, sqrt, both triangles and the
 * diagonal; per u the diversity.
 * workspace >= eg_take_distance_workspace_bytes(frames, U, R), which is 0 for arguments the call would refuse.
 * Refuses by name, before the first launch: null pointers, feat / workspace / distance / diversity not 16-byte aligned, U outside
 * 1 .. 65535, draws outside 2 .. EG_TAKE_MAX_DRAWS, frames[u] < 1, K < 4 or not a multiple of 4, N * K >= 2^40, a short workspace.
 * Both calls: one stream, no allocation, no host round trip, no synchronisation; launches, grids and pointers are fixed for a fixed
 * (frames, draws), so they capture into a hipGraph. */
#define EG_TAKE_CHUNK_FRAMES 16
#define EG_TAKE_MAX_DRAWS 64
int64_t eg_take_meta_ints(int32_t recordings);
int eg_take_meta(const int32_t* frames, int32_t recordings, int32_t* meta);
int eg_track_rows_pack(const float* track, int32_t recordings, int32_t draws, int32_t Tmax, int32_t pose_dim, const int32_t* frames,
                       const int32_t* d_meta, float* rows, void* stream);
int64_t eg_take_distance_workspace_bytes(const int32_t* frames, int32_t recordings, int32_t draws);
int eg_take_distance(const float* feat, int32_t recordings, int32_t draws, int32_t feat_dim, const int32_t* frames, const int32_t* d_meta,
                     int32_t span /* <= 0: none */, void* workspace, int64_t workspace_bytes, double* distance, double* diversity,
                     void* stream);

/* Emotion recognition of whole tracks: does a take show the emotion it was asked for?  The whole-track counterpart of the eval loop's
 * Emotion_ACC (test_emotion_gesture_diversity_iterative.py:216-221: the skeleton emotion classifier on the generated poses), for tracks of
 * any and unequal length with R takes each (csrc/emotion.hip).  The classifier itself (skeleton_classifer/Models.py:199-283) is eg_linear,
 * eg_multi_head_attention and eg_positionwise_ffn; these entries are everything around it.
 *
 * Classifier windows.  A window is F = the classifier's n_position consecutive poses of one take: no padding, no resampling.  Recording u
 * with frames[u] valid poses and stride S >= 1 has windows at 0, S, 2S, ... while start + F <= frames[u]; with tail != 0 one more at
 * frames[u] - F when (frames[u] - F) % S != 0, so that every valid pose is seen.  C_u is that count; frames[u] < F is refused by name.
 * Clip order: recording-major, then take, then window: clip R * coff[u] + r * C_u + j, coff the exclusive prefix sum of C;
 * N = R * sum(C_u).  Poses at or beyond frames[u] are never read.
 * Meta table (host only: no HIP call, usable without a GPU): eg_emotion_meta writes `frames | off | C | coff`, 4U int32 (the count
 * eg_emotion_meta_ints returns; 0 for U outside 1 .. 65535), and returns N / R = sum(C_u), or 0 for refused arguments.  Refuses by name: null
 * pointers, U outside 1 .. 65535, frames[u] < F, F < 1, S < 1, sum(frames) >= 2^31 (C_u <= frames[u], so the window counts are in range with the frames).
 *
 * eg_emotion_window_embed.  emb [R * sum(frames), d_model] fp32 is the classifier's per-pose embedding (prior_seq_encoder.fc1, fc2: run once
 * per valid pose, not once per window) in the packed order of eg_track_rows_pack; pos [F, d_model] the encoder's positional table.  For
 * the clip range [c0, c1):   x[(c - c0) * F + f, k] = emb[R*off[u] + r*frames[u] + start(u, j) + f, k] + pos[f, k]
 * -- the gather of the windows and the encoder's first row addition in one pass, one IEEE fp32 addition per element.  One launch gridded over
 * the chip, every output element has one owning thread, 16-byte loads and stores.  The range only bounds the caller's workspace: an element
 * of x does not depend on it.  Refuses by name: null pointers, emb / pos / x not 16-byte aligned, d_model not a multiple of 4, draws outside
 * 1 .. EG_TAKE_MAX_DRAWS, c0 < 0, c1 > N, an empty range, and what the meta call refuses.
 *
 * eg_emotion_vote on all logits [N, C] fp32, 2 <= C <= EG_EMOTION_MAX_CLASSES, from counts[u] = C_u (HOST, each >= 1) and d_counts, a device
 * copy of `C | coff` (2U int32: the second half of the meta table).  Per window i: valid(i) = all C logits finite; window_class[i] = the
 * lowest index among the maxima when valid, -1 otherwise.  Per take (u, r) with n = C_u windows:
 *   votes[u, r, c]       int32   valid windows of class c
 *   invalid[u, r]        int32   windows that are not valid
 *   mean_logit[u, r, c]  fp64    (sum over valid windows of the widened fp32 logits) / valid count; the sum runs over ascending windows
 *                                inside a chunk of EG_EMOTION_CHUNK_WINDOWS windows, then over ascending chunks (it may depend on that
 *                                constant and on nothing else); NaN when no window is valid.  Against the exact mean the error is at most
 *                                (n + 2) * 2^-53 * sum |l| / count.
 *   pred[u, r]           int32   the class with the most votes; among tied classes the larger mean_logit; still tied, the lowest index;
 *                                -1 when no window is valid
 * With d_labels (int32 [U * R] on the device, may be NULL; then the seven label outputs may be NULL too and are not written):
 *   hit[u, r] = pred == y;   window_hits[u, r] = votes[u, r, y];   accuracy = 100 * sum hit / (U R);
 *   window_accuracy = 100 * sum window_hits / N  (fp64, in percent);   confusion [C, C] int32: row = label, column = pred, over takes with
 *   pred >= 0;   window_confusion [C, C]: row = label, column = window_class, over valid windows.
 * unscored (int32, always written): takes with pred == -1.
 * The device cannot refuse a label: labels are trusted to lie in [0, C) (a host caller checks them before the upload).  A label outside
 * the range is never used as an index: such a take has hit = window_hits = 0, enters no cell of either matrix and counts in `unscored` only.
 * Two launches.  Stage 1: one wave per (take, chunk): the class of every window, the chunk's fp64 logit sums and int32 counts ->
 * workspace.  Stage 2: one wave per take adds its chunks in ascending order; one further workgroup walks all takes in ascending order for
 * the pooled figures.  No atomics, no memset, no allocation, no host round trip; grids and pointers are fixed for fixed (counts, draws, C),
 * so the call captures into a hipGraph.  workspace >= eg_emotion_vote_workspace_bytes (0 for arguments the call would refuse).
 * Refuses by name, before the first launch: null pointers, workspace not 16-byte aligned, fp64 outputs not 8-byte aligned, U outside
 * 1 .. 65535, draws outside 1 .. EG_TAKE_MAX_DRAWS, C outside 2 .. EG_EMOTION_MAX_CLASSES, counts[u] < 1, N >= 2^31, a short workspace. */
#define EG_EMOTION_CHUNK_WINDOWS 64
#define EG_EMOTION_MAX_CLASSES 64
int64_t eg_emotion_meta_ints(int32_t recordings);
int64_t eg_emotion_meta(const int32_t* frames, int32_t recordings, int32_t window, int32_t stride, int32_t tail, int32_t* meta);
int eg_emotion_window_embed(const float* emb, const float* pos, int32_t recordings, int32_t draws, int32_t window, int32_t stride,
                            int32_t tail, int32_t d_model, const int32_t* frames, const int32_t* d_meta, int32_t c0, int32_t c1, float* x,
                            void* stream);
int64_t eg_emotion_vote_workspace_bytes(const int32_t* counts, int32_t recordings, int32_t draws, int32_t classes);
int eg_emotion_vote(const float* logits, int32_t recordings, int32_t draws, int32_t classes, const int32_t* counts, const int32_t* d_counts,
                    const int32_t* d_labels, void* workspace, int64_t workspace_bytes, int32_t* window_class, int32_t* votes,
                    int32_t* invalid, double* mean_logit, int32_t* pred, int32_t* hit, int32_t* window_hits, double* accuracy,
                    double* window_accuracy, int32_t* confusion, int32_t* window_confusion, int32_t* unscored, void* stream);

/* Motion-clip features of whole tracks: the convolutional tower of MotionAE's encoder (model/motion_ae.py: PoseEncoderConv.net, the feature
 * net behind the TED-style Frechet gesture distance) on every 34-frame window of tracks of any and unequal length with R takes each, in one
 * launch (csrc/motionfeat.hip).  The three Linears behind it (out_net) are eg_linear products on the rows this entry writes.
 *
 * Windows, clip order and the `frames | off | C | coff` table are those of eg_emotion_meta with window = EG_MOTION_WINDOW: the caller uploads
 * that table once per (frames, stride, tail) and passes the device copy as d_frames (its first U entries are the frames) beside the host vector.
 * track [U, R, Tmax, D] fp32; poses at or beyond frames[u] are never read and may hold NaN.
 * Weights: four (w [cout, cin, k], bias [cout]) pairs in PyTorch's Conv1d layout with the BatchNorm already folded in:
 *   D -> 32, k 3, LeakyReLU(0.2);   32 -> 64, k 3, LeakyReLU;   64 -> 64, k 4, stride 2, LeakyReLU;   64 -> 32, k 3, plain
 * (34 -> 32 -> 30 -> 14 -> 12 positions).  For the clip range [c0, c1):   rows[c - c0, co * 12 + l] = the last layer's output (co, l) of clip
 * c -- [c1 - c0, EG_MOTION_ROW_FLOATS], the flatten(1) layout out_net consumes.  The range only bounds the caller's workspace: an element of
 * rows does not depend on it.
 * Arithmetic: every output element of every layer is bias first, then one fp32 multiply-add per term with ci ascending and k inner, then the
 * LeakyReLU -- eg_conv1d's order, so the rows equal the chain of four eg_conv1d calls on host-cut windows bit for bit.
 * Kernel: a workgroup owns a run of eg_motion_run_windows(stride) consecutive strided windows of one take (the tail window is a run of its
 * own) and stages at most EG_MOTION_RUN_FRAMES poses for it, channel-major, once; the first two layers (stride 1, no padding: shift-
 * invariant) run once per position of the run, not once per window; the last two run per window in batches or, where the windows of a run
 * overlap enough (small strides), once per position too: output l of the window at pose s is position s + 2l of one stride-1 pass, shared
 * by all windows of one start parity.  The weights are staged layer by layer; activations never leave the LDS.  No atomics, no memset, no allocation, no host round trip; grid and pointers are fixed for fixed
 * (frames, draws, stride, tail, range), so the launch captures into a hipGraph.
 * Refuses by name, before the launch: null pointers, track / rows not 16-byte aligned, U outside 1 .. 65535, draws outside
 * 1 .. EG_TAKE_MAX_DRAWS, D outside 1 .. EG_MOTION_MAX_POSE_DIM, window != EG_MOTION_WINDOW, stride < 1, frames[u] < window or > Tmax,
 * N >= 2^31, c0 < 0, c1 > N, an empty range, and a d_frames the rows contract refuses (not 4-byte aligned). */
#define EG_MOTION_WINDOW 34
#define EG_MOTION_ROW_FLOATS 384
#define EG_MOTION_MAX_POSE_DIM 128
#define EG_MOTION_RUN_FRAMES 136
int32_t eg_motion_run_windows(int32_t stride);
int eg_motion_window_rows(const float* track, int32_t recordings, int32_t draws, int32_t Tmax, int32_t pose_dim, int32_t window,
                          int32_t stride, int32_t tail, const int32_t* frames, const int32_t* d_frames, const float* w1, const float* b1,
                          const float* w2, const float* b2, const float* w3, const float* b3, const float* w4, const float* b4, int32_t c0,
                          int32_t c1, float* rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * Block-level operators (the reference's L2 blocks), used by the module-level mirrors and by the
 * per-kernel parity tests.  Weights here are passed as individual device pointers in the PACKED
 * layouts named above.
 * ------------------------------------------------------------------------------------------ */

/* nn.Conv2d 3x3 pad 1 (Full_model/ResNetBlocks.py:12,14; ResNetSE34V2.py:21) on NHWC fp32 with the
 * fused epilogue  v = acc + bias[c]; if relu: v = max(v,0); v = v*scale[c] + shift[c].
 *   x [B,H,W,Cin]   w EG_PACK_CONV3X3   bias/scale/shift [Cout_pad] (NULL = 0/1/0)
 *   Cout_pad = eg_conv3x3_cout_pad(Cin, Cout, stride): the padded width of the kernel that serves the shape, NOT round_up(Cout, 16) -- 128 -> 1..48
 *   reads rows of 48 and 128 -> 65..128 rows of 128.  The weight image is packed at that row length (zero columns past Cout) and all three vectors
 *   have that many readable elements.
 *   y NHWC [B,Ho,Wo,Cout] or, if nchw_out, [B,Cout,Ho*Wo]
 *   gap_partial (optional) [B, eg_conv3x3_gap_tiles(...), Cout]: per-tile channel sums of y (for SE).
 * The stride-2 stage entries (32 -> 64, 64 -> 128, split-bf16 modes, NHWC) run on parity planes with 4- or 8-row tiles once the launch fills the
 * chip (EG_CONV_S2 = interleaved | planes | planes4 | planes8 forces a form); their partials stay one per 2 x 32 output block in either form.
 * Served (Cin, stride, Cout): (32, 1, 17..32) (32, 2, 49..64) (64, 1, 49..64) (64, 2, 113..128) (64, 1, 128) (128, 1, 1..128) (128, 2, 241..256)
 * (256, 1, 256); anything else returns EG_ERR_UNSUPPORTED before a launch.  (64, 1, 113..127) and (256, 1, 241..255) launched until round 14, on a
 * grid of 4- and 2-row tiles over partials that eg_conv3x3_gap_tiles counts in 8- and 4-row tiles: wrong results, now refused. */
int eg_conv3x3(const float* x, const float* w, const float* bias, const float* scale, const float* shift,
               float* y, float* gap_partial, int32_t batch, int32_t h, int32_t wdt, int32_t cin, int32_t cout,
               int32_t stride, int32_t relu, int32_t nchw_out, int32_t precision, void* stream);
int32_t eg_conv3x3_gap_tiles(int32_t h, int32_t wdt, int32_t cin, int32_t cout, int32_t stride);
/* Cout_pad of eg_conv3x3 and of every entry point that shares its dispatch: a multiple of 16, >= cout; 0 where no kernel serves (cin, stride, cout). */
int32_t eg_conv3x3_cout_pad(int32_t cin, int32_t cout, int32_t stride);
/* The output-channel split (1, 2 or 4 workgroups per pixel tile) the NHWC convolution takes at this shape and precision: the split kernels
 * serve the bf16x3 stride-1 64 -> 64 and 128 -> 128 bodies while there are few pixel tiles (EG_CONV_SPLIT forces 1, 2 or 4). */
int32_t eg_conv3x3_channel_split(int32_t batch, int32_t h, int32_t wdt, int32_t cin, int32_t cout, int32_t stride, int32_t precision);
/* eg_conv3x3 with the SEBasicBlock tail of an identity block fused into the epilogue (ResNetBlocks.py:28-36):
 *   y = relu(BN(conv(x)) * gate[b, co] + residual[pixel, co]),   gate [B, Cout] from eg_se_gate_pre, residual NHWC like y.
 * gate == residual == NULL: plain eg_conv3x3.  gate == NULL with a residual: y = BN(conv(x)) + residual, no ReLU -- the fused fan-in add of
 * the training path (an input gradient landing on a tensor that has a second consumer). */
int eg_conv3x3_se(const float* x, const float* w_packed, const float* bias, const float* scale, const float* shift, const float* gate,
                  const float* residual, float* y, float* gap_partial, int32_t batch, int32_t h, int32_t wdt, int32_t cin, int32_t cout,
                  int32_t stride, int32_t relu, int32_t nchw_out, int32_t precision, void* stream);
/* y = conv(x) + (bit ? residual : 0), stride 1, NHWC: the input gradient of an SEBasicBlock's first convolution with the identity shortcut's
 * gradient dout * [out > 0] (ResNetBlocks.py:33-36 under autograd) added in the epilogue from `dout` and the tail's ReLU bit mask (eg_se_tail_forward's
 * relu_bits: bit e & 31 of word e >> 5 for element e) -- the masked map is never stored (eg_se_tail_backward_apply with dres == NULL).
 * x = the upstream gradient, w_packed = the flipped filter image (eg_pack_conv3x3_device with flip_transpose). */
int eg_conv3x3_res_masked(const float* x, const float* w_packed, const float* residual, const uint32_t* res_bits, float* y, int32_t batch, int32_t h,
                          int32_t wdt, int32_t cin, int32_t cout, int32_t precision, void* stream);
/* Training forward of a tower convolution (nn.Conv2d -> optional ReLU, ResNetBlocks.py:24-27 under autograd) in the split-bf16 modes: y as
 * eg_conv3x3 plus BOTH per-(clip, tile) channel partials, sums of y and of y*y ([batch][eg_conv3x3_gap_tiles][cout] each), so that the train-mode
 * BatchNorm that follows takes mean and variance from them (eg_bn_train_forward_sq) without reading y again. */
int eg_conv3x3_sq(const float* x, const float* w_packed, const float* bias, float* y, float* gap_partial, float* gap_sq_partial, int32_t batch,
                  int32_t h, int32_t wdt, int32_t cin, int32_t cout, int32_t stride, int32_t relu, int32_t precision, void* stream);
/* The same convolution on x' = x * in_scale[ci] + in_shift[ci] (per INPUT channel; in-image pixels only, the zero padding stays zero): the train-mode
 * BatchNorm in front of the convolution (ResNetBlocks.py:26-27, bn1 -> conv2) folded into the operand staging -- the normalised map is never written.
 * in_scale / in_shift come from eg_bn_train_stats_sq.  Split-bf16 modes, cin % 32 == 0.  gap_partial / gap_sq_partial: both or neither. */
int eg_conv3x3_sq_in_affine(const float* x, const float* in_scale, const float* in_shift, const float* w_packed, const float* bias, float* y,
                            float* gap_partial, float* gap_sq_partial, int32_t batch, int32_t h, int32_t wdt, int32_t cin, int32_t cout, int32_t stride,
                            int32_t relu, int32_t precision, void* stream);
/* SELayer gate of a block computed BEFORE its conv2 runs: the spatial mean of BN2(conv2(t1)) is linear in window sums of t1
 * (total from conv1's gap partials, border lines / corners read from t1), so gate = sigmoid(W2 relu(W1 mean + b1) + b2) needs
 * only t1 and conv2's fp32 weight image (the head of its EG_PACK_CONV3X3 entry).  t1 NHWC [B,H,W,C], conv2: C -> C, stride 1. */
int eg_se_gate_pre(const float* t1, const float* gap_partial, int32_t tiles, const float* conv2_w_packed, const float* scale2,
                   const float* shift2, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                   int32_t batch, int32_t h, int32_t wdt, int32_t c, void* stream);
/* One SEBasicBlock (ResNetBlocks.py:21-37) in the audio tower's fused data flow -- what eg_generator_forward runs per block when the SE fusion is on:
 *   t1 = BN1(relu(conv1(x)))  (stride 1 or 2, with per-tile channel sums in gap_partial)  ->  eg_se_gate_pre on t1  ->
 *   out = relu(gate * BN2(conv2(t1)) + shortcut) from conv2's epilogue.  Neither conv2's output y nor a shortcut map is written; three launches.
 * ds_w == NULL: identity shortcut (cin == cout, stride 1; any precision).  ds_w = the EG_PACK_CONV1X1_BF16 images of `downsample.0.weight`: the strided
 * 1x1 shortcut is contracted on the matrix pipe inside conv2 (split-bf16 modes only; 32 -> 64 and 64 -> 128), ds_scale / ds_shift its folded BatchNorm.
 *   x [B,H,W,Cin]; conv1_w, conv2_w EG_PACK_CONV3X3; scale / shift [Cout]; se_* as eg_se_gate
 *   scratch: t1 [B,Ho,Wo,Cout], gap_partial [B, eg_conv3x3_gap_tiles(H,W,Cin,Cout,stride), Cout], gate [B,Cout], sc_vec [3,B,Cout] (downsample only)
 *   out [B,Ho,Wo,Cout], distinct from x and t1. */
int eg_se_block_fused(const float* x, const float* conv1_w, const float* scale1, const float* shift1, const float* conv2_w, const float* scale2,
                      const float* shift2, const float* se_w1, const float* se_b1, const float* se_w2, const float* se_b2, const float* ds_w,
                      const float* ds_scale, const float* ds_shift, float* t1, float* out, float* gap_partial, float* gate, float* sc_vec,
                      int32_t batch, int32_t h, int32_t wdt, int32_t cin, int32_t cout, int32_t stride, int32_t precision, void* stream);
/* size in floats of one EG_PACK_CONV3X3 image (fp32 image + bf16 hi/lo images) */
int64_t eg_conv3x3_packed_floats(int32_t cin, int32_t cout_pad);

/* Stem: Conv2d(1->C,3x3,bias) -> ReLU -> BN (ResNetSE34V2.py:64-66).  x [B,H,W], y NHWC [B,H,W,C]. */
int eg_stem_conv(const float* x, const float* w9xc, const float* bias, const float* scale, const float* shift,
                 float* y, int32_t batch, int32_t h, int32_t wdt, int32_t c, void* stream);

/* SELayer gate (ResNetBlocks.py:92-96): s[b,c] = sigmoid(W2 relu(W1 mean_hw(y) + b1) + b2) from the
 * per-tile sums written by eg_conv3x3.  w1 [C/8,C], w2 [C,C/8] raw nn.Linear layouts. */
int eg_se_gate(const float* gap_partial, int32_t tiles, const float* w1, const float* b1, const float* w2,
               const float* b2, float* gate, int32_t batch, int32_t c, int32_t hw, void* stream);

/* SEBasicBlock tail (ResNetBlocks.py:28-36): out = relu(y*gate[b,c] + residual), residual = x_in or,
 * for the first block of a stage, BN(conv1x1_stride(x_in)) (ResNetSE34V2.py:43-47).
 *   y,out [B,Ho,Wo,C]; x_in [B,H,W,Cin]; ds_w EG_PACK_CONV1X1 or NULL. */
int eg_se_residual_relu(const float* y, const float* gate, const float* x_in, const float* ds_w,
                        const float* ds_scale, const float* ds_shift, float* out, int32_t batch, int32_t ho,
                        int32_t wo, int32_t c, int32_t h_in, int32_t w_in, int32_t cin, int32_t stride, void* stream);

/* nn.Linear family: Y[M,N] = epi(X[M,K] . W[N,K]^T).
 *   v = acc + bias[n] + res1[m,n];  if relu: v = max(v,0);  if res2: v = max(v + res2[m,n], 0)
 * lda/ldw/ldc/ldr in floats; K, lda, ldw multiples of 4 and X, W 16-byte aligned.
 * a_shift/a_seq implement the causal dilated tap of Full_model/tcn.py:18-24: source row of output row m is
 * m - a_shift, taken as zero when (m % a_seq) < a_shift (a_shift = 0 disables). */
int eg_linear(const float* x, int32_t lda, const float* w, int32_t ldw, const float* bias,
              const float* res1, const float* res2, int32_t ldr, float* y, int32_t ldc,
              int32_t m, int32_t n, int32_t k, int32_t relu, int32_t a_shift, int32_t a_seq,
              int32_t precision, void* stream);
/* Pre-split activations: eg_split_tiles converts fp32 X [M,K] into bf16 (hi, lo) tile-planar images
 * [ceil(M/64)][Kpad/8][64][8] (hi image then lo image; Kpad = K rounded up to 64; 4*ceil(M/64)*64*Kpad bytes);
 * eg_linear_presplit consumes them (same epilogue as eg_linear, bf16 modes only).  Used where one activation feeds several
 * products, so that it is split once instead of by every consuming workgroup. */
int eg_split_tiles(const float* x, int32_t lda, int32_t m, int32_t k, void* images, void* stream);
int eg_linear_presplit(const void* x_images, int32_t k_x, const float* w, int32_t ldw, const float* bias,
                       const float* res1, const float* res2, int32_t ldr, float* y, int32_t ldc,
                       int32_t m, int32_t n, int32_t k, int32_t relu, int32_t precision, void* stream);
/* A causal two-tap convolution over rows (tcn.py:18-24: pad d, chomp d) as ONE pre-split product:
 *   y[r] = epi(b + W0 x[r - shift] + W1 x[r]),  x[r - shift] = 0 where (r mod period) < shift,  epi = relu, then relu(. + res2) when res2 is given.
 * x_images: X [M, k_tap] as eg_split_tiles images of width k_x; w: the EG_PACK_LINEAR image of [W0 | W1] ([N][2*k_tap], each tap zero padded to
 * k_tap; ldw = 2*k_tap); zero_line: k_tap * 128 cleared bytes of device memory (the source of the rows that see zero).  The accumulator runs
 * through one K chain, tap 0 first.  y (fp32, may be NULL) and / or y_images (images of width y_k, may be NULL) receive the result.  bf16 modes. */
int eg_linear_presplit_causal(const void* x_images, int32_t k_x, const void* zero_line, const float* w, int32_t ldw, const float* bias,
                              const float* res2, int32_t ldr, float* y, int32_t ldc, void* y_images, int32_t y_k, int32_t m, int32_t n,
                              int32_t k_tap, int32_t relu, int32_t shift, int32_t period, int32_t precision, void* stream);

/* Split-K variant for tall-K, short-M products (emotion_classifer_header.0: K = frames*d_model,
 * Models_spatial_memory.py:500).  partial >= splits*M*N floats. */
int eg_linear_splitk(const float* x, int32_t lda, const float* w, int32_t ldw, const float* bias, float* y,
                     int32_t ldc, int32_t m, int32_t n, int32_t k, int32_t relu, int32_t splits,
                     float* partial, int32_t precision, void* stream);

/* The extended product of the TRAINING path: eg_linear / eg_linear_splitk plus the two element masks a train()-mode transformer block needs
 * around a product, so that they cost no launch of their own (Full_model/SubLayers.py:54,79: `q = self.dropout(self.fc(q)); q += residual`,
 * `x = self.dropout(x); x += residual`; Models_spatial_memory.py:488-536: the Dropout(0.2) between the Linears of the projection MLPs):
 *   v = acc + bias[n]
 *   gate_src:  v = gate_src[m,n] > 0 ? v : 0      -- ReLU backward fused into the input-gradient product (gate_src = the forward's ReLU output)
 *   drop_p>0:  v = keep(seed, epoch, drop_offset + m*n_cols + n) ? v / (1 - drop_p) : 0   -- nn.Dropout on the product; the mask is the counter
 *              hash of eg_dropout_dev on the flat [M, N] index, so a backward pass re-draws it (here or with eg_dropout_dev) from the same scalars
 *   v += res1[m,n];  relu;  res2 as eg_linear.
 * splits >= 2: split-K (partial >= splits*M*N floats) with the same epilogue applied by the fixed-order fold.
 * precision f32: w is [N, ldw] fp32; bf16 modes: the EG_PACK_LINEAR image (eg_pack_linear_device), ldw % 64 == 0. */
typedef struct EgLinearArgs {
    const float* x; const float* w; const float* bias; const float* res1; const float* res2; float* y;
    const float* gate_src;          /* [M, ldg] or NULL */
    const int32_t* drop_epoch;      /* device-resident step counter or NULL (eg_dropout_dev) */
    float* partial;                 /* split-K scratch or NULL */
    uint64_t drop_offset;
    int32_t lda, ldw, ldr, ldc, ldg;
    int32_t m, n, k, relu, precision, splits;
    uint32_t drop_seed;
    float drop_p;
} EgLinearArgs;
int eg_linear_ex(const EgLinearArgs* args, void* stream);

/* nn.LayerNorm(D, eps) over the last axis (Full_model/SubLayers.py:55-57,80-82).  rows x D, 1 <= D <= 2048 (else
 * EG_ERR_UNSUPPORTED); D % 4 == 0 takes the 16-byte kernel, any other D (the 282-wide discriminator) a scalar one with the same two-pass order. */
int eg_layernorm(const float* x, const float* gamma, const float* beta, float* y, int32_t rows, int32_t d,
                 float eps, void* stream);
/* The same with a second output: y as bf16 (hi, lo) tile-planar images [ceil(rows/64)][d/8][64][8] (eg_split_tiles layout, d % 64 == 0) for the
 * pre-split product that consumes the row next (y_images may be NULL). */
int eg_layernorm_img(const float* x, const float* gamma, const float* beta, float* y, void* y_images, int32_t rows, int32_t d, float eps,
                     void* stream);

/* ScaledDotProductAttention (Full_model/Modules.py:13-23) for all heads, mask=None, eval mode:
 * out[b,i,h*dv:(h+1)*dv] = softmax_j((q[b,i,h]/sqrt(dk)) . k[b,j,h]) v[b,j,h].
 * q [B,Lq,H*dk] (row stride ldq), k/v [B,Lk,H*dk] (ldk/ldv), out [B,Lq,H*dk] (ldo).  dk == 64.
 * attn (optional) [B,H,Lq,Lk] receives the probabilities (the reference returns them).
 * Both products run on MFMA in the arithmetic mode `precision` (EG_PREC_*); pointers 16-byte aligned, Lk <= 256. */
int eg_attention(const float* q, int32_t ldq, const float* k, int32_t ldk, const float* v, int32_t ldv,
                 float* out, int32_t ldo, float* attn, int32_t batch, int32_t heads, int32_t lq, int32_t lk,
                 int32_t dk, int32_t precision, void* stream);
/* The same with the reference's mask argument (Modules.py:18-19: `attn = attn.masked_fill(mask == 0, -1e9)` before the softmax): mask bytes
 * [batch][1 or lq][lk], 0 = masked; mask_query_stride = 0 broadcasts one key row per clip over the queries, else it is the byte distance of
 * consecutive query rows (>= lk); mask_batch_stride the byte distance of consecutive clips.  The head axis is broadcast, as
 * MultiHeadAttention.forward does with `mask.unsqueeze(1)` (SubLayers.py:44-45).  The gesture path itself always passes mask = None
 * (Models_spatial_memory.py:574,611); this entry exists so that Encoder / Decoder / MultiHeadAttention keep their full signature. */
int eg_attention_masked(const float* q, int32_t ldq, const float* k, int32_t ldk, const float* v, int32_t ldv, const uint8_t* mask,
                        int64_t mask_batch_stride, int32_t mask_query_stride, float* out, int32_t ldo, float* attn, int32_t batch,
                        int32_t heads, int32_t lq, int32_t lk, int32_t dk, int32_t precision, void* stream);

/* MultiHeadAttention.forward (Full_model/SubLayers.py:30-59): LN(fc(attn(q Wq, k Wk, v Wv)) + q).
 * xq [B*Lq, D], xkv [B*Lk, D]; wq/wk/wv packed nn.Linear [heads*64, D], wo packed [D, heads*64] (d_k = d_v = 64; D need not
 * equal heads*64: Motion_Discriminator runs D = 128 with 8 heads); out [B*Lq, D].  D % 4 == 0.
 * workspace >= eg_mha_workspace_bytes. */
int64_t eg_mha_workspace_bytes(int32_t batch, int32_t lq, int32_t lk, int32_t d_model, int32_t heads);
int eg_multi_head_attention(const float* xq, const float* xkv, const float* wq, const float* wk, const float* wv,
                            const float* wo, const float* ln_g, const float* ln_b, float* out, float* attn,
                            int32_t batch, int32_t lq, int32_t lk, int32_t d_model, int32_t heads,
                            int32_t precision, void* workspace, int64_t workspace_bytes, void* stream);

/* PositionwiseFeedForward.forward (Full_model/SubLayers.py:74-84): LN(w2 relu(w1 x + b1) + b2 + x). */
int64_t eg_ffn_workspace_bytes(int32_t rows, int32_t d_model, int32_t d_inner);
int eg_positionwise_ffn(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* ln_g, const float* ln_b, float* out, int32_t rows, int32_t d_model,
                        int32_t d_inner, int32_t precision, void* workspace, int64_t workspace_bytes, void* stream);

/* TemporalConvNet.forward (Full_model/tcn.py:63; TemporalBlock :43-47), channels-last:
 * x, y [B, L, C]; per level i (dilation 2^i) two weight-normed causal convs k=2 + ReLU, residual, ReLU.
 * w points at levels*2 convs, each {tap0 [C,Cpad], tap1 [C,Cpad], bias [C]} packed back to back
 * (EG_PACK_WN_TAP x2 + RAW); Cpad = C rounded up to 64.  workspace >= 4*B*L*Cpad floats. */
int eg_tcn_forward(const float* x, const float* w, float* y, int32_t batch, int32_t len, int32_t c,
                   int32_t levels, int32_t precision, void* workspace, int64_t workspace_bytes, void* stream);

/* eg_add_rows (below) that also writes the sum as eg_split_tiles images of width d (d % 64 == 0; 4*ceil(rows/64)*64*d bytes, rows past the last
 * one are left untouched): the producer-side split for the product that consumes the sum. */
int eg_add_rows_split(const float* a, const float* table, float* out, void* images, int64_t rows, int32_t d, int32_t period, void* stream);
/* out[r,:] = a[r,:] + table[r % period,:]  (PositionalEncoding.forward, Full_model/Models_spatial_memory.py:46-48);
 * period == 0: plain elementwise add of two [rows, d] tensors (fusion add, :601-605).  d % 4 == 0. */
int eg_add_rows(const float* a, const float* table, float* out, int64_t rows, int32_t d, int32_t period, void* stream);

/* TextEncoderTCN.fc1, a Linear over the time axis of channels-last rows (Full_model/Models_spatial_memory.py:164-166,176):
 * y[b,t',ch] = bias[t'] + sum_t w[t',t] x[b,t,ch];  x, y [batch, len, ld] with c <= ld used channels, w [len, len], bias [len].  Each output
 * element is summed bias first, then t ascending, one multiply-add per term.  len * (round_up(len, 4) + 64) floats of LDS must fit 64 KB
 * (len <= 99), else EG_ERR_UNSUPPORTED.
 * EG_TIME_LINEAR=ref (read per call) selects the one-row-at-a-time reference kernel; any other non-empty value is EG_ERR_BAD_ARG. */
int eg_time_linear(const float* x, const float* w, const float* bias, float* y, int32_t batch, int32_t len, int32_t c, int32_t ld, void* stream);

/* The front half of Prior_MemoryEncoder on its own (the generator calls the same launcher): Full_model/Models_spatial_memory.py:366-390 and, for
 * the memory variant, Full_model/Models_memory.py:233-251,282-293.  PL = frames - prior_frames.
 *   prior [batch, prior_frames, d];  conv: a HOST array of eight device pointers {w1 [PL, prior_frames, 3], b1, s1, t1 [PL], w2 [PL, PL, 3], b2, s2,
 *   t2 [PL]}: pred = BN2(ReLU(conv2(BN1(ReLU(conv1(prior)))))) with the prior frames as channels, the pose axis as the length (padding 1, the hidden
 *   map zero padded) and each eval-mode BatchNorm folded to y * s + t.
 *   mem: NULL or a HOST array of twelve device pointers, all NULL for variant 0 and all set for variant 1 (nn.Linear layouts):
 *   {sp_w0 [d, chunk d], sp_b0 [d], sp_w1 [d, d], sp_b1 [d], tc_w0, tc_b0, tc_w1, tc_b1 (the same shapes), tm_w0 [chunk, chunk d], tm_b0 [chunk],
 *   tm_w1 [chunk, chunk], tm_b1 [chunk]}.  Variant 1: m = sp1(sp0(flat(prior[:, P - chunk:]))), the first chunk frames of pred become
 *   s pred_c + (1 - s) m with s = sigmoid(<m, pred_c>);  tm_mem = tc1(tc0(the same flat chunk)),  tm_pe = tm1(tm0(flat(the gated frames))),
 *   tm_gram = tm_mem^T tm_pe (a sum over the BATCH: the clips of one call are coupled, as in the reference), w = softmax_c(tm_mem[b] tm_gram),
 *   pred_c = pred_c + pred_c w_c.
 *   cat [batch, frames, dpad] = cat(prior, pred) with the columns d .. dpad-1 written as +0;  tm_mem [batch, d], tm_pe [batch, chunk],
 *   tm_gram [d, chunk] (variant 1 only; may be NULL for variant 0, where chunk is ignored).
 * EG_ERR_BAD_ARG, by name: dpad < d; variant 1 with chunk outside 1 .. min(prior_frames, frames - prior_frames, 64) (the gated frames are
 * predicted ones, the scores live in 64 slots); memory pointers partly set, or not matching the variant.  EG_ERR_UNSUPPORTED: the slice of one
 * workgroup (variant 0: 64 pose columns; variant 1: the whole axis plus chunk d + 2 d floats) needs more than 160 KiB of LDS; the conv weights
 * are staged in LDS when they fit beside it and read from global memory otherwise.  Nothing is launched or written on a refusal. */
int eg_prior_encoder(const float* prior, const float* const* conv, const float* const* mem, float* cat, float* tm_mem, float* tm_pe, float* tm_gram,
                     int32_t batch, int32_t prior_frames, int32_t frames, int32_t d, int32_t dpad, int32_t chunk, int32_t variant, void* stream);

/* nn.Embedding gather into padded rows (Full_model/Models_spatial_memory.py:171): out[r, 0:dim] = table[clamp(idx[r], 0, n_words - 1)], bit for
 * bit; idx int64 [rows], table [n_words, dim], out [rows, ld].  dim % 4 == 0, ld >= dim, ld % 4 == 0 (else EG_ERR_ALIGN).
 * images == NULL: the columns dim .. ld-1 of out are left untouched.
 * images != NULL (ld % 64 == 0, else EG_ERR_ALIGN): the columns dim .. ld-1 are written as +0 and `images` receives the rows as eg_split_tiles
 * images of width ld (4 * ceil(rows/64) * 64 * ld bytes); the image slots of the last tile's rows past `rows` are left untouched.  zero_line
 * (optional, only with images): 64 * ld bf16 slots (128 * ld bytes) that are cleared -- the zero row source of the causal products that follow. */
int eg_embedding(const int64_t* idx, const float* table, float* out, void* images, void* zero_line, int32_t rows, int32_t dim, int32_t ld,
                 int32_t n_words, void* stream);

/* The CVAE's dense layers (CAVE/BEAT_CVAE.py: Posterior_Y_embedding, fusion_z_*): y[r, o] = bias[o] + sum_i w[o, i] x[r, i] for r < n, o < out;
 * x rows ldx >= in floats apart, y rows ldy >= out apart (the columns out .. ldy-1 of y are untouched), w [out, in].  One wave per output: lane l
 * sums i = l, l + 64, ... in ascending order, the 64 partials by a butterfly, the bias last.  n <= 65535. */
int eg_small_linear(const float* x, int32_t ldx, const float* w, const float* bias, float* y, int32_t ldy, int32_t n, int32_t in, int32_t out,
                    void* stream);

/* nn.ConvTranspose1d(k 3, stride 2, padding 1, output_padding 1) -> LeakyReLU(0.2) -> y * scale[co] + shift[co] (the CVAE decoder's stages,
 * CAVE/BEAT_CVAE.py:355-362): x [n, cin, lin] -> y [n, cout, 2 lin], w [cin, cout, 3] (PyTorch layout);
 * y[co, lo] = bias[co] + sum_ci sum_k x[ci, (lo + 1 - k) / 2] w[ci, co, k] over the k with lo + 1 - k even and 0 <= (lo + 1 - k) / 2 < lin:
 * a term outside that range is dropped, not multiplied by zero.  Summed bias first, ci outer, k inner.  scale and shift are required. */
int eg_conv_transpose1d(const float* x, const float* w, const float* bias, const float* scale, const float* shift, float* y, int32_t n, int32_t cin,
                        int32_t cout, int32_t lin, void* stream);

/* VAE reparameterisation (CAVE/BEAT_CVAE.py:397-399): z = eps*exp(0.5*logvar) + mu, n elements. */
int eg_reparameterize(const float* mu, const float* logvar, const float* eps, float* z, int64_t n, void* stream);

/* nn.Conv1d over [n, cin, lin] -> [n, cout, lout], lout = (lin + 2*pad - k)/stride + 1, weight [cout, cin, k] (PyTorch layout):
 * y = bias + conv(x);  if act != 0: y = LeakyReLU(0.2)(y);  if scale != NULL: y = y*scale[co] + shift[co].  The two steps are independent:
 * act == 0 with a scale applies the affine to the plain convolution (scale and shift come together, else EG_ERR_BAD_ARG).  act + scale is the
 * CVAE's conv -> LeakyReLU -> BN order (CAVE/BEAT_CVAE.py:318-332); MotionAE's conv -> BN -> LeakyReLU (model/motion_ae.py:8-31) folds its BN
 * into w / bias.
 * The input tile and the weights of one workgroup must fit 160 KB of LDS (else EG_ERR_UNSUPPORTED). */
int eg_conv1d(const float* x, const float* w, const float* bias, const float* scale, const float* shift, float* y, int32_t n,
              int32_t cin, int32_t cout, int32_t lin, int32_t k, int32_t stride, int32_t pad, int32_t act, void* stream);

/* SoftmaxContrastiveLoss (test_emotion_gesture_diversity_iterative.py:80-127), forward and evaluate in one call.
 * face, audio: [n, d] fp32.  Rows are L2-normalised (x / max(|x|, 1e-12)), cross[i][j] = max(1 / (|face_i - audio_j| + 1e-8), 1e-8),
 * loss = mean_i( logsumexp_j cross[i][j] - cross[i][i] )  (= F.cross_entropy(cross, arange(n))),  acc = mean_i( argmax_j cross[i][j] == i ).
 * cross ([n, n]) may be NULL; loss and acc are single floats on the device.  ws: eg_contrastive_workspace_bytes(n).
 * Deterministic: per-row results are reduced in a fixed order (no atomics).  1 <= n <= 4096, 1 <= d. */
int64_t eg_contrastive_workspace_bytes(int32_t n);
int eg_contrastive_loss(const float* face, const float* audio, int32_t n, int32_t d, float* cross, float* loss, float* acc,
                        void* workspace, int64_t workspace_bytes, void* stream);
/* Gradients of that loss (mode 'max') with respect to both feature sets, for an upstream gradient of 1: softmax of every row of cross_dist,
 * back through 1/(D + 1e-8), the pairwise distances and F.normalize.  workspace >= eg_contrastive_backward_workspace_bytes(n). */
int64_t eg_contrastive_backward_workspace_bytes(int32_t n);
int eg_contrastive_loss_backward(const float* face, const float* audio, int32_t n, int32_t d, float* gface, float* gaudio, void* workspace,
                                 int64_t workspace_bytes, void* stream);


/* ===================== training-path primitives (fp32, deterministic reductions) =====================
 * The reference trains through autograd over ATen (its one loop: train_audio_classifier_K_fold.py:155-175; generator
 * hints: test_emotion_gesture_diversity_iterative.py:64-127,355-366).  These are the backward-side kernels; the host
 * (emotiongestures_amd/train/) sequences them.  All buffers caller-owned, row-major, fp32. */

/* y[c*ldy + r] = x[r*ldx + c] */
int eg_transpose(const float* x, int32_t ldx, int32_t rows, int32_t cols, float* y, int32_t ldy, void* stream);
/* C[m,n] (+)= sum_k A[k,m] B[k,n] on v_mfma_f32_16x16x4_f32 (dW = dY^T X; conv wgrad over im2col rows); split-K through
 * `workspace` (eg_gemm_tn_workspace_floats; at least m*n floats when accumulate != 0). */
int64_t eg_gemm_tn_workspace_floats(int32_t m, int32_t n, int64_t k);
int eg_gemm_tn(const float* a, int32_t lda, const float* b, int32_t ldb, float* c, int32_t ldc, int32_t m, int32_t n, int64_t k,
               float* workspace, int64_t workspace_floats, int32_t accumulate, void* stream);
/* weight gradient of a 3x3 / pad 1 / stride s convolution as an implicit TN GEMM over the output pixels (no im2col buffer):
 * dw_mat [Cout][(kh*3+kw)*Cin + ci]; Cin % 4 == 0; workspace >= eg_gemm_tn_workspace_floats(cout, 9*cin, B*Ho*Wo) */
int eg_conv3x3_wgrad(const float* x, const float* dy, float* dw_mat, int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout,
                     int32_t stride, float* workspace, int64_t workspace_floats, void* stream);
/* 3x3 / pad 1 / stride s, NHWC: forward  col[(b,oy,ox)][tap*C + c] = x[b, oy*s+kh-1, ox*s+kw-1, c];
 * backward (x = dcol, col = dx [B,H,W,C]): the transpose in gather form (F.conv2d's input gradient after the GEMM). */
int eg_im2col3x3(const float* x, float* col, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t stride, int32_t backward, void* stream);
/* pixel subsample of a 1x1 stride-s conv (ResNetSE34V2.py:43-47) and its transpose */
int eg_subsample(const float* x, float* y, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t stride, int32_t backward, void* stream);
/* The small 1-D convolutions of the training step (emotion CVAE Conv1d / ConvTranspose1d stacks, CAVE/BEAT_CVAE.py:318-332,355-369; the prior
 * encoder's pred_conv, Full_model/Models_spatial_memory.py:224-231) on channels-last activations, one fp32 launch per product, fixed-order sums:
 *   forward          y[b, lo, co]  = bias[co] + sum_{ci, j} x[b, lo*stride - pad + j*dilation, ci] * w[co][ci][j]     (w: nn.Conv1d's [cout][cin][k])
 *   backward_input   dx[b, li, ci] = bias[ci] + sum_{co, j : li + pad - j*dilation = lo*stride} dy[b, lo, co] * w[co][ci][j]
 *   backward_weight  dw[co][ci][j] = sum_{b, lo} dy[b, lo, co] * x[b, lo*stride - pad + j*dilation, ci];  db_dy[co] = sum dy;  db_x[ci] = sum x
 * x / dx: [batch, len, cin], y / dy: [batch, len_out, cout]; bias, db_dy, db_x may be NULL; 1 <= k <= 8.  nn.ConvTranspose1d (weight
 * [cin][cout][k]) is the adjoint: forward = backward_input with the layer's bias, input gradient = forward, weight gradient = backward_weight
 * with x and dy exchanged (db_x = the layer's bias gradient). */
int eg_conv1d_cl_forward(const float* x, const float* w, const float* bias, float* y, int32_t batch, int32_t len, int32_t cin, int32_t len_out,
                         int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t dilation, void* stream);
int eg_conv1d_cl_backward_input(const float* dy, const float* w, const float* bias, float* dx, int32_t batch, int32_t len, int32_t cin,
                                int32_t len_out, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t dilation, void* stream);
/* workspace: eg_conv1d_cl_backward_weight_workspace_floats(...) floats (0 for small shapes: one launch); per-workgroup partials, folded in a fixed
 * order by a second launch.  db_x != NULL always takes the one-launch kernel. */
int64_t eg_conv1d_cl_backward_weight_workspace_floats(int32_t batch, int32_t cin, int32_t len_out, int32_t cout, int32_t k, int32_t stride,
                                                      int32_t dilation);
int eg_conv1d_cl_backward_weight(const float* x, const float* dy, float* dw, float* db_dy, float* db_x, int32_t batch, int32_t len, int32_t cin,
                                 int32_t len_out, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t dilation, float* workspace,
                                 int64_t workspace_floats, void* stream);
/* [rows, k] -> [rows, k_padded] zero padded (rows of the GEMM operands are read in 16-byte pieces) */
int eg_pad_cols(const float* x, float* y, int64_t rows, int32_t k, int32_t k_padded, void* stream);
/* nn.BatchNorm{1,2}d in train() mode over channels-last rows [rows, C]: batch statistics (biased variance for the
 * normalisation, unbiased for running_var, momentum as torch), saved mean / rstd for the backward.  The mean is taken in two steps (the centred
 * pass also sums the residuals about the first-pass mean and corrects it): its error scales with a channel's spread, not with its magnitude. */
int64_t eg_colreduce_workspace_floats(int32_t c);
int eg_bn_train_forward(const float* x, const float* gamma, const float* beta, float* y, float* save_mean, float* save_rstd,
                        float* running_mean, float* running_var, int64_t rows, int32_t c, float momentum, float eps, float* workspace,
                        void* stream);
/* relu_mask != 0: x is the output of a ReLU (conv1 -> ReLU -> bn1, ResNetBlocks.py:24-26) and dx is that ReLU's input gradient, dx * [x > 0]. */
int eg_bn_train_backward(const float* x, const float* dy, const float* gamma, const float* save_mean, const float* save_rstd, float* dx,
                         float* dgamma, float* dbeta, int64_t rows, int32_t c, int32_t relu_mask, float* workspace, void* stream);
/* BatchNorm (train mode) on a map that eg_conv3x3 just wrote together with gap_partial [batch][tiles][c] (per-tile channel sums): the mean
 * and clip_sum [batch][c] (nullable) come from the partials, one centred pass over x gives the variance and corrects the mean.  y NULL:
 * statistics only. */
int eg_bn_train_forward_gap(const float* x, const float* gap_partial, int32_t tiles, int32_t batch, const float* gamma, const float* beta,
                            float* y, float* save_mean, float* save_rstd, float* clip_sum, float* running_mean, float* running_var,
                            int64_t rows, int32_t c, float momentum, float eps, float* workspace, void* stream);
/* The same with the variance also from partials (eg_conv3x3_sq's sums of squares): two small launches, no pass over x; the per-tile partials are
 * fp32, everything across tiles / clips and E[x^2] - mean^2 is double (relative error of the variance ~1e-6 (1 + mean^2 / var): used in the
 * split-bf16 modes only).  x may be NULL when y is NULL. */
int eg_bn_train_forward_sq(const float* x, const float* gap_partial, const float* gap_sq_partial, int32_t tiles, int32_t batch, const float* gamma,
                           const float* beta, float* y, float* save_mean, float* save_rstd, float* clip_sum, float* running_mean, float* running_var,
                           int64_t rows, int32_t c, float momentum, float eps, float* workspace, void* stream);
/* Statistics only (no apply), plus the apply folded to one affine per channel: aff_scale = gamma * rstd, aff_shift = beta - mean * aff_scale -- for
 * eg_conv3x3_sq_in_affine / eg_conv3x3_wgrad_mfma_oihw_in_affine, which apply it while staging their operand. */
int eg_bn_train_stats_sq(const float* gap_partial, const float* gap_sq_partial, int32_t tiles, int32_t batch, const float* gamma, const float* beta,
                         float* save_mean, float* save_rstd, float* running_mean, float* running_var, float* aff_scale, float* aff_shift, int64_t rows,
                         int32_t c, float momentum, float eps, float* workspace, void* stream);
/* SEBasicBlock tail under autograd (ResNetBlocks.py:28-36,92-96), maps [batch, hw, c] channels-last, c % 8 == 0, c <= 256:
 *   forward:  pooled = mean_hw(bn2(c2)) from clip_sum; h = relu(W1 pooled + b1); gate = sigmoid(W2 h + b2)      (eg_se_gate_train_forward)
 *             out = relu(bn2(c2) * gate + res) in one pass, bn2's output never stored                            (eg_se_tail_forward)
 *   backward: one masked reduction pass (s1, s2raw per clip), the gate's backward per clip (dz2, dz1, dgap_hw, u1, u2), the sums over
 *             clips (bn2 / SE parameter gradients, m1, m2), and one apply pass writing dc2 and dres. */
int eg_se_gate_train_forward(const float* clip_sum, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* w1,
                             const float* b1, const float* w2, const float* b2, float* pooled, float* h, float* gate, int32_t batch, int32_t hw,
                             int32_t c, void* stream);
/* relu_bits (optional, batch * hw * c / 32 words; needs batch * hw * c % 32 == 0): the tail's ReLU mask [out > 0] as one nibble per float4 of the
 * map, eight float4 indices per word.  The two backward passes take it INSTEAD of `out` (then `out` may be NULL): they read 1/32 of a map where
 * they read a whole one (3.4 GB of the 128-clip step's 78).  eg_se_tail_backward_apply: dres may be NULL when relu_bits is given -- the consumer of
 * the shortcut's gradient then masks `dout` itself (eg_conv3x3_res_masked). */
int eg_se_tail_forward(const float* c2, const float* res, const float* mean, const float* rstd, const float* gamma, const float* beta,
                       const float* gate, float* out, uint32_t* relu_bits, int32_t batch, int32_t hw, int32_t c, void* stream);
int eg_se_tail_backward_reduce(const float* dout, const float* out, const uint32_t* relu_bits, const float* c2, const float* mean, float* s1,
                               float* s2raw, int32_t batch, int32_t hw, int32_t c, float* workspace, void* stream);
int eg_se_gate_train_backward(const float* s1, const float* s2raw, const float* clip_sum, const float* mean, const float* rstd,
                              const float* gamma, const float* beta, const float* gate, const float* h, const float* w1, const float* w2,
                              float* dz2, float* dz1, float* dgap_hw, float* u1, float* u2, int32_t batch, int32_t hw, int32_t c, void* stream);
int eg_se_tail_backward_finish(const float* u1, const float* u2, const float* dz2, const float* dz1, const float* h, const float* pooled,
                               float* dgamma, float* dbeta, float* m1, float* m2, float* dw1, float* db1, float* dw2, float* db2,
                               int32_t batch, int32_t hw, int32_t c, void* stream);
int eg_se_tail_backward_apply(const float* dout, const float* out, const uint32_t* relu_bits, const float* c2, const float* mean, const float* rstd,
                              const float* gamma, const float* gate, const float* dgap_hw, const float* m1, const float* m2, float* dc2, float* dres,
                              int32_t batch, int32_t hw, int32_t c, void* stream);
/* o0[c] = sum_r a[r,c]; o1[c] = sum_r a[r,c]*b[r,c] (b NULL: sum a^2).  bias / LayerNorm affine gradients. */
int eg_colsum(const float* a, const float* b, float* o0, float* o1, int64_t rows, int32_t c, float* workspace, void* stream);
/* op: 0 relu(a) | 1 a*(b>0) | 2 leaky(a; s) | 3 a*(b>0 ? 1 : s) | 4 a+b | 5 a*s | 6 sigmoid(a) | 7 a*b*(1-b) | 8 a*b | 9 a+s*b | 10 exp(s*a) | 11 a*b[0] */
int eg_elementwise(const float* a, const float* b, float* y, int64_t n, int32_t op, float s, void* stream);
/* The same weight gradient for stride 1 on the split-bf16 matrix pipe (x and dy split to hi/lo bf16 while staged, 3 MFMA terms, fp32
 * accumulation, fixed-order partial sums): cin % 32 == 0, cout % 32 == 0.  workspace >= eg_conv3x3_wgrad_mfma_workspace_floats(...). */
int64_t eg_conv3x3_wgrad_mfma_workspace_floats(int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout);
int eg_conv3x3_wgrad_mfma(const float* x, const float* dy, float* dw_mat, int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout,
                          float* workspace, int64_t workspace_floats, void* stream);
/* The same gradient written in nn.Conv2d's weight layout dw[cout][cin][3][3] by the final fixed-order reduction (no permute pass behind it). */
int eg_conv3x3_wgrad_mfma_oihw(const float* x, const float* dy, float* dw, int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout,
                               float* workspace, int64_t workspace_floats, void* stream);
/* ... of a convolution whose input was x' = x * in_scale[ci] + in_shift[ci] (eg_conv3x3_sq_in_affine): the affine is re-applied while x is staged. */
int eg_conv3x3_wgrad_mfma_oihw_in_affine(const float* x, const float* in_scale, const float* in_shift, const float* dy, float* dw, int32_t batch, int32_t h,
                                         int32_t w, int32_t cin, int32_t cout, float* workspace, int64_t workspace_floats, void* stream);
/* Input gradient of nn.Conv2d(cin -> cout, k = 3, pad = 1, stride = 2) -- the `_make_layer` entry convolutions, Full_model/ResNetSE34V2.py:40-55 (F.conv2d's
 * dgrad under autograd) -- on the split-bf16 matrix pipe, phase-decomposed: each dx pixel (2i + py, 2j + px) only receives the taps whose parity
 * matches (9 tap products per four pixels).  dy [batch][ho][wo][cout] NHWC with ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1; w_flip = the packed
 * images of the rotated, transposed filter (eg_pack_conv3x3 with flip = 1: what the stride-1 input gradients read); dx [batch][h][w][cin], every
 * element written.  res_q (optional, [batch][ho][wo][cin]): a gradient that belongs to the pixels (2i, 2j) of dx -- the input gradient of the
 * stride-2 1x1 shortcut (:43-47), which reads exactly those pixels -- added in the epilogue instead of being scattered into a zero map first.
 * precision: EG_PREC_BF16X3 only; (cin, cout) in {(32, 64), (64, 128), (128, 256)}; else EG_ERR_UNSUPPORTED. */
int eg_conv3x3_dgrad_s2(const float* dy, const float* w_flip, const float* res_q, float* dx, int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout,
                        int32_t precision, void* stream);
/* Weight and bias gradient of nn.Linear on the split-bf16 matrix pipe (3 x v_mfma_f32_16x16x32_bf16 per product, fp32 accumulate):
 *   dw[n][k] = sum_r dy[r][n] * x[r][k]   (dy [rows, n] at pitch ldy, x [rows, k] at pitch ldx, dw at pitch lddw);  db[n] = sum_r dy[r][n] (db may be NULL).
 * F.linear's parameter gradients under autograd (every nn.Linear of Full_model/Models_spatial_memory.py, SubLayers.py:30-84).  Deterministic: rows
 * are split over workgroups only through fixed-order partials in `workspace` (eg_linear_wgrad_mfma_workspace_floats floats; 0 = not needed). */
int64_t eg_linear_wgrad_mfma_workspace_floats(int32_t rows, int32_t n, int32_t k);
int eg_linear_wgrad_mfma(const float* dy, int32_t ldy, const float* x, int32_t ldx, float* dw, int32_t lddw, float* db, int32_t rows, int32_t n, int32_t k,
                         float* workspace, int64_t workspace_floats, void* stream);
/* Weight gradient of nn.Conv2d(cin -> cout, k = 3, pad = 1, stride 1 | 2) on the split-bf16 matrix pipe as dW = dY^T im2col(x), the im2col matrix gathered
 * from the NHWC map while the operand is staged (no column buffer): the stride-2 stage-entry convolutions, Full_model/ResNetSE34V2.py:40-55 (the stride-1
 * body convolutions keep eg_conv3x3_wgrad_mfma).  dy [batch][ho][wo][cout], dw_mat [cout][9 * cin] ((kh, kw, ci) fastest to slowest, as eg_conv3x3_wgrad).
 * cin % 4 == 0.  workspace >= eg_linear_wgrad_mfma_workspace_floats(batch * ho * wo, cout, 9 * cin).  Deterministic (fixed-order partials). */
int eg_conv3x3_wgrad_gather_mfma(const float* x, const float* dy, float* dw_mat, int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout,
                                 int32_t stride, float* workspace, int64_t workspace_floats, void* stream);
/* Device-side build of the weight image eg_conv3x3 reads (eg_conv3x3_packed_floats(cin', round_up(cout',16)) floats: fp32 image, then the
 * bf16 hi / lo images), for weights that change every step.  flip_transpose = 0: conv weight [cout][cin][3][3] as in the state_dict
 * (cin' = cin, cout' = cout).  flip_transpose = 1: the filter of the input-gradient convolution, w'[ci][co][kh][kw] = w[co][ci][2-kh][2-kw]
 * (cin' = cout, cout' = cin) -- F.conv2d's dgrad for stride 1 is eg_conv3x3 of dy with that image.  The rows are round_up(cout', 16) wide: the image
 * serves eg_conv3x3 only where eg_conv3x3_cout_pad(cin', cout', stride) is that width (not 128 -> 1..32 and 128 -> 65..112). */
int eg_pack_conv3x3_device(const float* w_oihw, int32_t cout, int32_t cin, int32_t flip_transpose, float* image, void* stream);
/* Device-side build of the weight image eg_linear's split-bf16 modes read (EG_PACK_LINEAR layout; eg_linear_packed_floats(n, k) floats,
 * ldw = k rounded up to 64) from w [n][k] fp32 with row stride ld.  transpose != 0: the image of w^T (w is then [k][n]): dX = dY W. */
int64_t eg_linear_packed_floats(int32_t n, int32_t k);
int eg_pack_linear_device(const float* w, int32_t ld, int32_t n, int32_t k, int32_t transpose, float* image, void* stream);
/* Every weight image of a training step in one launch.  `table`: device array of `count` 40-byte entries
 *   { const float* src; float* image; int32_t kind, a, b, c, flag, first_block; }
 * kind 0 = eg_pack_linear_device(src, ld = c, n = a, k = b, transpose = flag & 1, image); kind 1 = eg_pack_conv3x3_device(src, cout = a, cin = b, flip = flag & 1, image);
 * flag bit 1 set: the fp32 head of that image is left unwritten (only the split-bf16 kernels may read it);
 * first_block = sum of eg_pack_table_blocks(kind, a, b, flag) over the preceding entries, total_blocks = the sum over all. */
int32_t eg_pack_table_blocks(int32_t kind, int32_t a, int32_t b, int32_t flag);
int eg_pack_table(const void* table, int32_t count, int32_t total_blocks, void* stream);
/* nn.Dropout in train() mode with a counter-based mask (nothing stored): keep(i) = hash(seed, offset + i) >= p, y = keep ? x/(1-p) : 0;
 * the backward pass is the same call on dy.  The mask stream is this library's own (not torch's RNG). */
int eg_dropout(const float* x, float* y, int64_t n, float p, uint32_t seed, uint64_t offset, void* stream);
/* The same with a device-resident step counter mixed into the seed (epoch_dev may be NULL = eg_dropout): a training step replayed from a
 * captured hipGraph freezes the host scalars (seed, offset), the counter (incremented once per step by eg_counter_add inside the graph)
 * still gives every replay a fresh mask.  Forward and backward of one step read the same counter value. */
int eg_dropout_dev(const float* x, float* y, int64_t n, float p, uint32_t seed, uint64_t offset, const int32_t* epoch_dev, void* stream);
/* SELayer pieces (ResNetBlocks.py:92-96) on x [B, HW, C]: pooled mean (x scale), per-(clip, channel) dot, gate scaling (+ add[b,c]);
 * workspace (eg_colreduce_workspace_floats(c) floats) selects the two-level reduction, NULL the one-block-per-clip kernel */
int eg_seg_mean(const float* x, float* out, int32_t batch, int32_t hw, int32_t c, float scale, float* workspace, void* stream);
int eg_seg_dot(const float* dy, const float* x, float* out, int32_t batch, int32_t hw, int32_t c, float* workspace, void* stream);
int eg_se_scale(const float* a, const float* gate, const float* add, float* y, int32_t batch, int32_t hw, int32_t c, void* stream);
/* LayerNorm backward (SubLayers.py:55-57,80-82): dx and xhat; the affine gradients are one column reduction,
 * (dbeta, dgamma) = (sum dy, sum dy*xhat) = eg_colsum(dy, xhat, dbeta, dgamma, ...) */
int eg_layernorm_backward(const float* x, const float* dy, const float* gamma, float* dx, float* xhat, int32_t rows, int32_t d, float eps,
                          void* stream);
/* LayerNorm backward for the fused transformer blocks of the training path: dx as eg_layernorm_backward, the affine gradients from the SAME pass
 * (per-workgroup partial column sums + one fixed-order fold: no xhat round trip, no separate column reduction), and -- drop_p > 0 -- a second
 * output dx_dropped = nn.Dropout's backward applied to dx (the gradient that continues into the Dropout'ed branch `dropout(fc(.))` while dx itself
 * goes to the residual; mask = eg_dropout_dev's on the flat [rows, d] index).  d % 64 == 0, d <= 1024.  workspace: eg_layernorm_backward_ex_workspace_floats. */
int64_t eg_layernorm_backward_ex_workspace_floats(int32_t rows, int32_t d);
int eg_layernorm_backward_ex(const float* x, const float* dy, const float* gamma, float* dx, float* dx_dropped, float* dgamma, float* dbeta,
                             int32_t rows, int32_t d, float eps, float drop_p, uint32_t drop_seed, uint64_t drop_offset, const int32_t* epoch_dev,
                             float* workspace, void* stream);
/* Training pair on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32) with nn.Dropout(p) on the probabilities (Modules.py:21) from the counter-based
 * mask of eg_dropout (counter = offset + linear index of (clip, head, query, key); epoch_dev as in eg_dropout_dev, may be NULL).  The forward stores
 * the UNMASKED probabilities in `attn` [batch, heads, lq, lk]; the backward recomputes the mask from the same (p, seed, offset, epoch).  The backward
 * walks the queries in chunks with K / V resident in LDS: lk <= 128 (TED 34, BEAT 60, BEAT-long 120), any lq.  p = 0 is plain attention. */
int eg_attention_train(const float* q, int32_t ldq, const float* k, int32_t ldk, const float* v, int32_t ldv, float* out, int32_t ldo, float* attn,
                       int32_t batch, int32_t heads, int32_t lq, int32_t lk, int32_t dk, float p, uint32_t seed, uint64_t offset,
                       const int32_t* epoch_dev, void* stream);
int eg_attention_backward_train(const float* q, int32_t ldq, const float* k, int32_t ldk, const float* v, int32_t ldv, const float* attn,
                                const float* dout, int32_t ldo, float* dq, int32_t lddq, float* dk, int32_t lddk, float* dv, int32_t lddv,
                                int32_t batch, int32_t heads, int32_t lq, int32_t lk, int32_t dk_dim, float p, uint32_t seed, uint64_t offset,
                                const int32_t* epoch_dev, void* stream);
/* losses: scale * mean smooth-L1 (beta); scale * mean CE / focal(alpha[b] per sample or NULL, gamma >= 0)
 * (train_audio_classifier_K_fold.py:95-105: `alpha * (1-pt)**gamma * ce` broadcasts alpha over the batch axis) */
int eg_smooth_l1(const float* pred, const float* target, float* loss, float* dpred, int64_t n, float beta, float scale, float* workspace,
                 void* stream);
int eg_cross_entropy(const float* logits, const int64_t* labels, const float* alpha, float gamma, float scale, float* loss, float* dlogits,
                     int32_t batch, int32_t classes, float* workspace, void* stream);
/* VAE KL term of MLP_Reconstruct_v3's (mu, logvar) (CAVE/BEAT_CVAE.py:389-399,403-424): scale * mean_b(-0.5 sum_j(1 + lv - mu^2 - e^lv)) and its gradients */
int eg_kld(const float* mu, const float* logvar, float* loss, float* dmu, float* dlogvar, int32_t n, int32_t d, float scale, void* stream);
/* torch.optim.Adam step on a flat buffer (L2 weight decay added to the gradient; train_audio_classifier_K_fold.py:128) */
int eg_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int32_t step, void* stream);
/* The same update with the (1-based) step count read from device memory, and the counter's increment, for steps replayed from a captured
 * hipGraph (host scalars are frozen at capture). */
int eg_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, const int32_t* step_dev, void* stream);
int eg_counter_add(int32_t* counter, int32_t delta, void* stream);
/* The memory nets of Full_model/Models_memory.py's Prior_MemoryEncoder under autograd (the MLPs around them are ordinary Linear operators).
 * SP_Memory_Net_v1.forward (:233-251): for the first `chunk` of the `frames` predicted frames  s = sigmoid(<mem_b, pred_bc>),
 * out_bc = s pred_bc + (1 - s) mem_b; later frames pass through (mem [batch, dim], pred / out [batch, frames, dim], gate [batch, chunk] saved
 * for the backward, which returns dpred and dmem).
 * TM_Memory_Net.forward (:288-292) behind its batch-coupled score [batch, chunk] = mem (mem^T pe):  w = softmax(score, dim=1),
 * out_bc = pred_bc (1 + w_bc) for c < chunk; the backward returns dpred and dscore. */
int eg_sp_gate_forward(const float* mem, const float* pred, float* out, float* gate, int32_t batch, int32_t frames, int32_t dim, int32_t chunk, void* stream);
int eg_sp_gate_backward(const float* mem, const float* pred, const float* gate, const float* dout, float* dpred, float* dmem, int32_t batch,
                        int32_t frames, int32_t dim, int32_t chunk, void* stream);
int eg_tm_scale_forward(const float* score, const float* pred, float* out, float* w, int32_t batch, int32_t frames, int32_t dim, int32_t chunk, void* stream);
int eg_tm_scale_backward(const float* w, const float* pred, const float* dout, float* dpred, float* dscore, int32_t batch, int32_t frames, int32_t dim,
                         int32_t chunk, void* stream);
/* Gradient-bucket payload conversion for the data-parallel all-reduce (bf16 buckets, 79 MB instead of 158 MB per step over
 * xGMI): fp32 -> bf16 round-to-nearest-even, and bf16 -> fp32 times `scale`. */
int eg_f32_to_bf16(const float* x, uint16_t* y, int64_t n, void* stream);
int eg_bf16_to_f32(const uint16_t* x, float* y, int64_t n, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMOGEST_H */
