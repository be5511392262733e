// Audio tower kernels: stem conv, 3x3 implicit-GEMM conv on MFMA, SE gate, SE tail (+1x1 downsample).
// Reference semantics: Full_model/ResNetSE34V2.py:62-74, Full_model/ResNetBlocks.py:21-37,81-96.
//
// Data layout in HBM: activations NHWC fp32 (channel innermost, 128 B per pixel at C=32), so that
// the implicit-GEMM K axis (tap, channel) is contiguous per pixel and every global access is a
// 16-byte-per-lane coalesced load/store.
//
// conv3x3 kernel shape (one workgroup = 4 waves = TH x 32 output pixels x all output channels):
//   D[co][pix] = sum_{tap,ci} Wt[tap][ci][co] * X[pix + tap][ci]            (swapped operands)
//   A operand = weights  (lane: co = lane&15, k-quad = lane>>4), streamed from L2 (every workgroup
//                          reads the same <= 590 KB, so they stay cache resident),
//   B operand = pixels   (lane: pix = lane&15, k-quad = lane>>4), read from an LDS halo tile kept in a
//                          channel-quad planar image [ci/4][pixel][4]: a ds_read_b128 per lane, bank-conflict
//                          free for 16 consecutive pixels (plane stride = 0 mod 16 slots, stride 1; odd, stride 2),
//   D: each lane owns 4 consecutive output channels of one pixel -> one 16-byte NHWC store per tile.
#include <string.h>
#include <type_traits>
#include "common.h"

// (Measured and dropped in round 1: s_setprio around the MFMA cluster costs 20-50 % here -- hipcc stops interleaving the LDS
//  reads; a persistent 32->32 kernel with register-resident weights was 35 % slower than the tiled one.  Round 2's persistent 32->32
//  kernel below keeps the weights in LDS and the next tile's pixels in registers instead.)

namespace {

struct ConvArgs {
    const float* x; const float* w; const float* bias; const float* scale; const float* shift;
    float* y; float* gap;
    float* gap2 = nullptr;              // training forward: per-(clip, tile) channel sums of v*v beside `gap` (BatchNorm's variance without a pass over y)
    int H, W, Ho, Wo, cout, relu, nchw, tiles_x, tiles;
    // fused SE tail (SEBasicBlock.forward, ResNetBlocks.py:28-36, identity shortcut): v = relu(v * gate[b, co] + res[pixel, co])
    // applied after the BatchNorm affine; gate comes from se_gate_pre_kernel (computed BEFORE this convolution runs)
    const float* gate = nullptr; const float* res = nullptr; int relu2 = 0;
    // training: a per-INPUT-channel affine applied while the halo tile is staged (the BatchNorm in front of this convolution folded into its operand
    // staging: x' = x * in_scale[ci] + in_shift[ci] for pixels inside the image, zero padding stays zero) -- split-bf16 kernels only
    const float* in_scale = nullptr; const float* in_shift = nullptr;
    int wrow = 0;                       // channel-split launches: row length of the weight images (the convolution's padded output channels)
    const unsigned* res_bits = nullptr; // residual behind a ReLU mask: one bit per element of `res` (bit e & 31 of word e >> 5 = the nibble-per-float4 layout
                                        // se_tail_fwd_kernel writes): v += bit ? res : 0 -- the SE block's identity shortcut gradient dout * (out > 0), never stored
    const float* res_q = nullptr;       // DG2 only: a gradient on the dy grid ([B][H][W][cout]) added to the (even, even) phase -- the stride-2 1x1 shortcut's
    // conv2 of a block WITH a downsample shortcut (conv3x3_bf16_kernel, SCC > 0): the 1x1 stride-sc_S convolution of the block input sc_x
    // [B][sc_H][sc_W][SCC * 32] is contracted into the same accumulators before the 3x3 taps (weight images [ci/8][co][8], hi then lo) and the
    // per-clip vectors of se_gate_pre_kernel fold gate, BN2 and the shortcut's BN into one rescale and one affine: sc_vec = [f | q | h], each [B][cout]
    const float* sc_x = nullptr; const bf8* sc_whi = nullptr; const bf8* sc_wlo = nullptr; const float* sc_vec = nullptr;
    int sc_H = 0, sc_W = 0, sc_S = 2, sc_B = 0;             // sc_B: the batch (the stride between f, q and h is sc_B * cout)
};
// a quad of the residual, behind its ReLU bit mask when there is one (e = element index of the quad's first float, a multiple of 4)
__device__ __forceinline__ f4 residual_quad(const float* __restrict__ res, const unsigned* __restrict__ bits, size_t e) {
    f4 r = *reinterpret_cast<const f4*>(res + e);
    if (bits) {
        const unsigned nb = bits[e >> 5] >> (unsigned)(e & 28);
        r[0] = (nb & 1u) ? r[0] : 0.f;
        r[1] = (nb & 2u) ? r[1] : 0.f;
        r[2] = (nb & 4u) ? r[2] : 0.f;
        r[3] = (nb & 8u) ? r[3] : 0.f;
    }
    return r;
}

template <int S, int TH> struct ConvGeom {
    static constexpr int IH = (TH - 1) * S + 3;
    static constexpr int IW = 31 * S + 3;
    static constexpr int NPIX = IH * IW;
    static constexpr int PL = (S == 1) ? ((NPIX + 15) / 16 * 16) : (NPIX | 1);
    static constexpr int MT = TH * 2 / 4;
};

// Input gradient of a STRIDE-2 convolution (conv3x3_bf16_kernel, DG2): the tile is TH x 32 pixels of dy; a base pixel (i, j) owns the four dx pixels
// (2i + py, 2j + px) and needs dy at (i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1): halo of one row / column on the HIGH side only.
template <int TH> struct ConvGeomDG2 {
    static constexpr int IH = TH + 1;
    static constexpr int IW = 33;
    static constexpr int NPIX = IH * IW;
    static constexpr int PL = (NPIX + 15) / 16 * 16;
};

constexpr int WRING = 3;        // slots of the split-bf16 kernels' weight ring: step s runs, step s + 1's fragments are read, the copy of step s + 2 is in flight
// LDS of a kernel with a weight ring, in bf8 slots: [tile: NIMG images x 4 octet planes x PL pixels][WRING x WBUF: the NIMG weight images of a K step, 4 octet rows x COUTP]
template <int PL, int COUTP, int TERMS> struct RingLds {
    static constexpr int NIMG = (TERMS == 3) ? 2 : 1;
    static constexpr int TILE = NIMG * 4 * PL, WIMG = 4 * COUTP, WBUF = NIMG * WIMG;
    static constexpr size_t BYTES = sizeof(bf8) * (size_t)(TILE + WRING * WBUF);
};
template <int S, int TH, bool DG2> using ConvBf16Geom = typename std::conditional<DG2, ConvGeomDG2<TH>, ConvGeom<S, TH>>::type;     // conv3x3_bf16_kernel's halo tile

// Tap order of the STRIDE-2 split-bf16 convolutions: by the (row, column) parity of the input pixel a tap reads, which is the order the parity-plane
// walk of the stage entries needs (conv3x3_s2_planes_kernel).  The interleaved form (conv3x3_bf16_kernel, S = 2) accumulates in the same order, so that
// the two forms -- chosen by the size of the launch -- give every output element bit for bit the same value.
constexpr int s2p_tap(int k) { constexpr int T[9] = {4, 3, 5, 1, 7, 0, 2, 6, 8}; return T[k]; }        // tap of the chunk's k-th step
constexpr int s2p_plane(int k) { constexpr int P[9] = {0, 1, 1, 2, 2, 3, 3, 3, 3}; return P[k]; }      // its plane = (row parity) * 2 + (column parity)

// the three-term split-bf16 product of a fragment pair, small terms first: acc += wl * xh + wh * xl + wh * xh (TERMS == 1: the last term alone)
template <int TERMS> __device__ __forceinline__ f4 mfma_split(bf8 wh, bf8 wl, bf8 xh, bf8 xl, f4 acc) {
    if (TERMS == 3) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, xh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xl, acc, 0, 0, 0);
    }
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xh, acc, 0, 0, 0);
}
__device__ __forceinline__ f4 relu4(f4 v) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
    return v;
}
// 8 staged fp32 channels of one pixel -> the tile's hi image (and, for the three-term product, its lo image 4 planes behind)
template <int TERMS, int PL> __device__ __forceinline__ void store_split(bf8* tile, int slot, const f4& v0, const f4& v1) {
    bf8 hi, lo;
    split_octet<TERMS == 3>(v0, v1, hi, lo);
    tile[slot] = hi;
    if (TERMS == 3) tile[4 * PL + slot] = lo;
}
// staging roles of the split-bf16 kernels by thread index: 8 consecutive lanes stage 8 consecutive pixels of one channel octet (conflict-free ds_write_b128)
__device__ __forceinline__ int stage_pixel(int idx) { return (idx >> 5) * 8 + (idx & 7); }
__device__ __forceinline__ int stage_octet(int idx) { return (idx >> 3) & 3; }
// a wave's fragments of one K step, and the read of their weight half: Wh = the lane's first slot in the step's hi image, the lo image lies WIMG slots behind
template <int NT, int MT> struct ConvFrags { bf8 wh[NT], wl[NT], xh[MT], xl[MT]; };
template <int TERMS, int WIMG, int NT, int MT> __device__ __forceinline__ void read_w_frags(ConvFrags<NT, MT>& f, const bf8* Wh) {
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        f.wh[n] = Wh[n * 16];
        if (TERMS == 3) f.wl[n] = Wh[WIMG + n * 16];
    }
}

// ---- fp32 MFMA path -------------------------------------------------------------------------
template <int CIN, int NT, int S, int TH>
__global__ __launch_bounds__(256) void conv3x3_f32_kernel(ConvArgs a) {
    using G = ConvGeom<S, TH>;
    constexpr int COUTP = NT * 16, IW = G::IW, NPIX = G::NPIX, PL = G::PL, MT = G::MT;
    __shared__ f4 tile[8 * PL];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, kq = lane >> 4;
    // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs, so give each XCD a contiguous run of tiles
    // (whole clips at B >= 8); halo rows / columns shared by neighbouring tiles then hit in that XCD's L2.
    int tile_id = blockIdx.x, b = blockIdx.y;
    {
        const int total = gridDim.x * gridDim.y;
        if ((total & 7) == 0) {
            const int lin = blockIdx.y * gridDim.x + blockIdx.x;
            const int log = (lin & 7) * (total >> 3) + (lin >> 3);
            b = log / (int)gridDim.x;
            tile_id = log - b * (int)gridDim.x;
        }
    }
    const int ty = tile_id / a.tiles_x, tx = tile_id - ty * a.tiles_x;
    const int oy0 = ty * TH, ox0 = tx * 32;
    const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;

    int pbase[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int id = wave * MT + t;
        pbase[t] = ((id >> 1) * S) * IW + ((id & 1) * 16 + li) * S;
    }
    f4 acc[MT][NT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[t][n] = (f4){0.f, 0.f, 0.f, 0.f};

    const f4* __restrict__ w4 = reinterpret_cast<const f4*>(a.w);
    const float* __restrict__ xb = a.x + (size_t)b * a.H * a.W * CIN;

    for (int chunk = 0; chunk < CIN / 32; ++chunk) {
        if (chunk) __syncthreads();
        // stage the (IH x IW) x 32-channel halo tile: 8 consecutive lanes = 8 consecutive pixels of one
        // channel quad (conflict-free ds_write_b128); a wave still covers 8 pixels x 128 contiguous bytes.
        for (int idx = tid; idx < ((NPIX + 7) / 8) * 64; idx += 256) {
            const int p = (idx >> 6) * 8 + (idx & 7), cq = (idx >> 3) & 7;
            if (p < NPIX) {
                const int iy = p / IW, ix = p - iy * IW;
                const int gy = iy0 + iy, gx = ix0 + ix;
                f4 v = (f4){0.f, 0.f, 0.f, 0.f};
                if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
                    v = *reinterpret_cast<const f4*>(xb + ((size_t)gy * a.W + gx) * CIN + chunk * 32 + cq * 4);
                tile[cq * PL + p] = v;
            }
        }
        __syncthreads();
        const f4* wp = w4 + (size_t)(chunk * 8 + kq) * COUTP + li;
#pragma unroll 1
        for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int tap = kh * 3 + kw, toff = kh * IW + kw;
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    f4 wv[NT], xv[MT];
#pragma unroll
                    for (int n = 0; n < NT; ++n) wv[n] = wp[(size_t)(tap * (CIN / 4) + g * 4) * COUTP + n * 16];
#pragma unroll
                    for (int t = 0; t < MT; ++t) xv[t] = tile[(g * 4 + kq) * PL + pbase[t] + toff];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int t = 0; t < MT; ++t)
#pragma unroll
                            for (int n = 0; n < NT; ++n)
                                acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[n][j], xv[t][j], acc[t][n], 0, 0, 0);
                }
            }
        }
    }

    // ---- epilogue: v = acc + bias; relu?; v*scale + shift; NHWC f4 store / NCHW scalar store; SE sums
    f4 gsum[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) gsum[n] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int co = n * 16 + kq * 4;
        const f4 bi = a.bias ? *reinterpret_cast<const f4*>(a.bias + co) : (f4){0.f, 0.f, 0.f, 0.f};
        const f4 sc = a.scale ? *reinterpret_cast<const f4*>(a.scale + co) : (f4){1.f, 1.f, 1.f, 1.f};
        const f4 sh = a.shift ? *reinterpret_cast<const f4*>(a.shift + co) : (f4){0.f, 0.f, 0.f, 0.f};
        const f4 gt = (a.gate && co < a.cout) ? *reinterpret_cast<const f4*>(a.gate + (size_t)b * a.cout + co) : (f4){1.f, 1.f, 1.f, 1.f};
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int id = wave * MT + t;
            const int oy = oy0 + (id >> 1), ox = ox0 + (id & 1) * 16 + li;
            const bool valid = (oy < a.Ho) && (ox < a.Wo);
            f4 v = acc[t][n] + bi;
            if (a.relu) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            }
            v = v * sc + sh;
            if (a.gate) v = v * gt;
            if (a.res && valid && co < a.cout) v += residual_quad(a.res, a.res_bits, (((size_t)b * a.Ho + oy) * a.Wo + ox) * a.cout + co);
            if (a.relu2) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            }
            if (valid) {
                if (!a.nchw) {
                    if (co < a.cout)
                        *reinterpret_cast<f4*>(a.y + (((size_t)b * a.Ho + oy) * a.Wo + ox) * a.cout + co) = v;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (co + r < a.cout)
                            a.y[((size_t)b * a.cout + co + r) * a.Ho * a.Wo + (size_t)oy * a.Wo + ox] = v[r];
                }
                gsum[n] += v;
            }
        }
    }
    if (a.gap) {
        float* sred = reinterpret_cast<float*>(tile);
        __syncthreads();                                      // all waves are done reading the halo tile
#pragma unroll
        for (int n = 0; n < NT; ++n) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float s = gsum[n][r];
                s = row16_sum(s);
                if (li == 0) sred[wave * COUTP + n * 16 + kq * 4 + r] = s;
            }
        }
        __syncthreads();
        if (tid < a.cout) {
            const float s = (sred[tid] + sred[COUTP + tid]) + (sred[2 * COUTP + tid] + sred[3 * COUTP + tid]);
            a.gap[((size_t)b * a.tiles + tile_id) * a.cout + tid] = s;
        }
    }
}

// ---- split-bf16 MFMA path (EG_PREC_BF16X3 / EG_PREC_BF16) --------------------------------------
// Same tiling, but BOTH operands come from LDS and the weight stream is asynchronous:
//  * halo tile: split while it is staged, hi = bf16(x), lo = bf16(x - hi), kept as two channel-octet planar images
//    [ci/8][pixel][8 bf16] (same 16-byte slot structure as the fp32 image => conflict-free ds_read_b128);
//  * weights: pre-split on the host into [tap][ci/8][co][8] (hi image, lo image).  The 4 octets of one (tap, 32-channel
//    chunk) are one contiguous 64*COUTP-byte run, copied by global_load_lds (16 B/lane, no VGPR, no VALU) into a
//    3-slot LDS ring two steps ahead; one barrier per step (placed mid-step, counted vmcnt: see the schedule comment
//    in the kernel) retires the copy of step s+1 while the copy of step s+2 stays in flight;
//  * waves tile the workgroup's TH x 32 pixels x COUTP channels as WM (pixels) x WN (channels); per step and
//    (pixel tile, channel tile) pair:  acc += Whi*Xhi + Whi*Xlo + Wlo*Xhi   (3 x v_mfma_f32_16x16x32_bf16).
// Without the LDS weight ring every wave re-read all weights from L1/L2 (170 B/clk/CU demanded at C=128 vs 64 B/clk
// of L1): the r01a profile's 115 us per 128->128 launch.

// SPLIT: the workgroup computes the NTT * 16 output channels starting at blockIdx.z * NTT * 16 of a convolution with a.cout channels in all (its
// weight images' row length `a.wrow`): small batches of the 64- and 128-channel stages have fewer pixel tiles than the chip has CUs (one clip: 8 tiles of
// 128 -> 128), so the channels are spread over workgroups too.  Same pixel -> (wave, tile, lane) map (WM, MT) and the same K order as the unsplit
// instantiation: every output element and every pooling partial is bitwise the same, whichever the launch function picks.
//
// DG2: the INPUT GRADIENT of a stride-2 convolution (F.conv2d's dgrad for the two `_make_layer` entry convolutions, ResNetSE34V2.py:40-55) on the same
// machinery, phase-decomposed: x here is dy [B][H][W][CIN] (CIN = the convolution's output channels: the contraction), y is dx [B][Ho][Wo][cout],
// Ho = the convolution's input height.  dx[2i + py][2j + px] only receives the taps whose parity matches: (even, even) 1 tap, (even, odd) / (odd, even)
// 2, (odd, odd) 4 -- 9 tap-products per FOUR output pixels instead of the 36 a zero-upsampled stride-1 convolution would issue.  One step is still one
// (tap, 32-channel chunk) with the same weight ring; it accumulates into the phase the tap belongs to (4 x the accumulators, hence the smaller
// tiles of the launch table).  The weight images are those of the rotated, transposed filter the stride-1 input gradients use (pack flip):
// image tap t' is the filter's tap (2 - t'/3, 2 - t'%3), which reads dy at (i + (t'/3 == 2), j + (t'%3 == 2)).
//
// SCC > 0: conv2 of a block whose shortcut is a strided 1x1 convolution of the block input (SCC 32-channel chunks of it; the `_make_layer` entries,
// ResNetSE34V2.py:43-47) with the WHOLE block tail in this launch: out = relu(gate * BN2(conv2(t1)) + BNd(conv1x1(x))) (ResNetBlocks.py:28-36).
// Before the 3x3 loop the workgroup stages its tile's shortcut pixels x[sc_S * oy, sc_S * ox] at the halo-tile positions the centre tap reads, one
// 32-channel chunk at a time, split to (hi, lo) like any halo, and runs one ordinary K step per chunk against the packed 1x1 images (the same
// [ci/8][co][8] packing with a single tap, in the weight ring's free slots).  The accumulators D are then rescaled in place by
// f[b][co] = sd[co] / q[b][co], q = gate[b][co] * s2[co], the 3x3 taps accumulate on top, and the epilogue relu(acc * q + h),
// h = h2 * gate + hd, yields gate * (conv2 * s2 + h2) + (D * sd + hd).  f, q, h come from se_gate_pre_kernel, which keeps |q| >= 1e-30.
//
// One workgroup computes one tile in one straight pass: prologue (first two weight copies, first halo chunk, the shortcut pre-phase when SCC > 0), the
// chunk x tap loop, the epilogue.
template <int CIN, int NTT, int S, int TH, int WM, int WN, int TERMS, bool SPLIT = false, bool DG2 = false, int SCC = 0>
__global__ __launch_bounds__(256, 2) void conv3x3_bf16_kernel(ConvArgs a, const bf8* __restrict__ whi,
                                                           const bf8* __restrict__ wlo) {
    static_assert(!DG2 || (S == 1 && !SPLIT), "DG2 tiles the dy grid with unit stride");
    static_assert(SCC == 0 || (S == 1 && !DG2 && SCC <= 2 && CIN >= 64), "the shortcut pre-phase belongs to a stride-1 conv2 and uses ring slots 2 and 1");
    using G = ConvBf16Geom<S, TH, DG2>;
    constexpr int PH = DG2 ? 4 : 1;                 // output phases (accumulator sets)
    constexpr int COUTP = NTT * 16, IW = G::IW, NPIX = G::NPIX, PL = G::PL;
    constexpr int MT = TH * 2 / WM, NT = NTT / WN;
    using L = RingLds<PL, COUTP, TERMS>;
    constexpr int NIMG = L::NIMG, TILE = L::TILE, WIMG = L::WIMG, WBUF = L::WBUF;
    constexpr int NSTEP = (CIN / 32) * 9;
    static_assert(WM * WN == 4 && MT * WM == TH * 2 && NT * WN == NTT, "wave tiling");
    extern __shared__ __attribute__((aligned(16))) bf8 lds[];      // RingLds: TILE + WRING * WBUF slots (dynamic: can exceed 64 KB)
    bf8* tile = lds;
    bf8* wring = lds + TILE;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, kq = lane >> 4;
    const int wm = wave / WN, wn = wave % WN;
    // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs, so give each XCD a contiguous run of tiles
    // (whole clips at B >= 8); halo rows / columns shared by neighbouring tiles then hit in that XCD's L2.
    int tile_id = blockIdx.x, b = blockIdx.y;
    const int c0 = SPLIT ? (int)blockIdx.z * COUTP : 0;        // first output channel of this workgroup
    if (!SPLIT) {
        const int total = gridDim.x * gridDim.y;
        if ((total & 7) == 0) {
            const int lin = blockIdx.y * gridDim.x + blockIdx.x;
            const int log = (lin & 7) * (total >> 3) + (lin >> 3);
            b = log / (int)gridDim.x;
            tile_id = log - b * (int)gridDim.x;
        }
    }
    const int oy0 = (tile_id / a.tiles_x) * TH, ox0 = (tile_id % a.tiles_x) * 32;

    int pbase[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int id = wm * MT + t;
        pbase[t] = ((id >> 1) * S) * IW + ((id & 1) * 16 + li) * S;
    }
    f4 acc[PH][MT][NT];
#pragma unroll
    for (int ph = 0; ph < PH; ++ph)
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[ph][t][n] = (f4){0.f, 0.f, 0.f, 0.f};
    const float* xb = a.x + (size_t)b * a.H * a.W * CIN;       // the clip whose halo load_tile fetches

    // one step's weights = NIMG runs of WIMG slots; 64-slot (1 KiB) pieces are dealt round-robin to the 4 waves
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    constexpr int PIECES = WIMG / 64;
    // (image, piece) pairs are dealt round-robin to the 4 waves as one flat list, so that every wave issues the same number
    // of copies per step whenever NIMG * PIECES is a multiple of 4 (then the per-step wait can be a counted vmcnt)
    constexpr int GTOT = NIMG * PIECES;
    constexpr bool COUNTED = (GTOT % 4 == 0);
    constexpr int GW = GTOT / 4;
    // one K step's weights: octet rows row0 .. row0 + 3 of the images (hi, lo) -> ring slot buf
    auto issue_rows = [&](const bf8* __restrict__ ihi, const bf8* __restrict__ ilo, int row0, int buf) {
        if constexpr (SPLIT) {
            // the slice's 4 octet rows of COUTP slots are not contiguous in the image (row length a.wrow): per-lane source addresses, the LDS side
            // stays one contiguous KiB per wave-instruction
            static_assert(COUNTED, "split instantiations deal whole pieces to the four waves");
            const size_t rbase = (size_t)row0 * a.wrow + c0;
#pragma unroll
            for (int p = 0; p < GW; ++p) {
                const int flat = p * 4 + wave_u;
                const int img = flat / PIECES, piece = flat - img * PIECES;
                const int slot = piece * 64 + lane, oct = slot / COUTP, co = slot - oct * COUTP;
                const bf8* src = (img ? ilo : ihi) + rbase + (size_t)oct * a.wrow + co;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(wring + buf * WBUF + img * WIMG + piece * 64), 16, 0, 0);
            }
            return;
        }
        const size_t gbase = (size_t)row0 * COUTP;
        if constexpr (PIECES % 4 == 0) {        // every wave copies PIECES / 4 pieces of each image (image known at compile time)
#pragma unroll
            for (int img = 0; img < NIMG; ++img) {
                const bf8* src = (img ? ilo : ihi) + gbase;
#pragma unroll
                for (int p = 0; p < PIECES / 4; ++p) {
                    const int piece = p * 4 + wave_u;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + piece * 64 + lane),
                                                     (__attribute__((address_space(3))) void*)(wring + buf * WBUF + img * WIMG + piece * 64),
                                                     16, 0, 0);
                }
            }
        } else {                                // few pieces: deal the flat (image, piece) list
#pragma unroll
            for (int p = 0; p < (GTOT + 3) / 4; ++p) {
                const int flat = p * 4 + wave_u;
                if (COUNTED || flat < GTOT) {
                    const int img = flat / PIECES, piece = flat - img * PIECES;
                    const bf8* src = (img ? ilo : ihi) + gbase;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + piece * 64 + lane),
                                                     (__attribute__((address_space(3))) void*)(wring + buf * WBUF + img * WIMG + piece * 64),
                                                     16, 0, 0);
                }
            }
        }
    };
    // the chunk's k-th step: taps 0 .. 8 in order, in plane order (s2p_tap) at stride 2
    auto tap_of = [](int k) { return (S == 2 && !DG2) ? s2p_tap(k) : k; };
    auto issue_weights = [&](int step, int buf) {
        const int chunk = step / 9, tap = tap_of(step - chunk * 9);
        issue_rows(whi, wlo, tap * (CIN / 8) + chunk * 4, buf);
    };
    // halo tile staging, split in two so the HBM latency of chunk c+1 hides under the 9 taps of chunk c:
    //   load_tile: (IH x IW) pixels x 32 channels -> registers (one lane = one pixel x 8 channels per iteration)
    //   store_tile: split to (hi, lo) bf16 and write the channel-octet planar LDS image
    constexpr int NIT = (((NPIX + 7) / 8) * 32 + 255) / 256;
    f4 pv[NIT][2];
    // per-lane staging roles are chunk independent: compute the global element offset (32-bit; -1 = zero padding / unused)
    // and the LDS slot once, so the per-chunk loops carry no address arithmetic
    int goff[NIT], lslot[NIT];
    auto set_goff = [&](int toy0, int tox0) {       // the halo of the tile whose first output pixel is (toy0, tox0)
        const int iy0 = DG2 ? toy0 : toy0 * S - 1, ix0 = DG2 ? tox0 : tox0 * S - 1;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = tid + it * 256;
            const int p = stage_pixel(idx), oc = stage_octet(idx);
            const int iy = p / IW, ix = p - iy * IW;
            const int gy = iy0 + iy, gx = ix0 + ix;
            const bool inside = p < NPIX && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            goff[it] = inside ? (gy * a.W + gx) * CIN + oc * 8 : -1;
            lslot[it] = p < NPIX ? oc * PL + p : -1;
        }
    };
    set_goff(oy0, ox0);
    auto load_tile = [&](int chunk) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            pv[it][0] = pv[it][1] = (f4){0.f, 0.f, 0.f, 0.f};
            if (goff[it] >= 0) {
                const float* src = xb + goff[it] + chunk * 32;
                pv[it][0] = *reinterpret_cast<const f4*>(src);
                pv[it][1] = *reinterpret_cast<const f4*>(src + 4);
            }
        }
    };
    const int oc8s = ((tid >> 3) & 3) * 8;          // this thread's channel octet inside a 32-channel chunk (the same for all its iterations)
    auto store_tile = [&](int chunk) {
        f4 s0 = (f4){1.f, 1.f, 1.f, 1.f}, s1 = s0, h0 = (f4){0.f, 0.f, 0.f, 0.f}, h1 = h0;
        const bool in_aff = a.in_scale != nullptr;
        if (in_aff) {
            s0 = *reinterpret_cast<const f4*>(a.in_scale + chunk * 32 + oc8s); s1 = *reinterpret_cast<const f4*>(a.in_scale + chunk * 32 + oc8s + 4);
            h0 = *reinterpret_cast<const f4*>(a.in_shift + chunk * 32 + oc8s); h1 = *reinterpret_cast<const f4*>(a.in_shift + chunk * 32 + oc8s + 4);
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (lslot[it] >= 0) {
                if (in_aff && goff[it] >= 0) {          // inside the image only: the zero padding of the normalised map stays zero
                    pv[it][0] = pv[it][0] * s0 + h0;
                    pv[it][1] = pv[it][1] * s1 + h1;
                }
                store_split<TERMS, PL>(tile, lslot[it], pv[it][0], pv[it][1]);
            }
        }
    };

    // glds instructions this wave issues per step (pieces are dealt round-robin, so it can differ by wave)
    // Schedule (3-slot weight ring, fragments double-buffered in registers, taps fully unrolled):
    //   step s:  issue the weight copy of step s+2  ->  read step s+1's fragments from LDS (in flight during ...)
    //            ... the MFMAs of step s  ->  vmcnt(0) + barrier (copies of s+1, s+2 landed; slot of s is free)
    // so neither the LDS fragment reads nor the global->LDS weight copies sit on the MFMA critical path.
    using Frags = ConvFrags<NT, MT>;
    auto read_w = [&](Frags& f, int slot) {                                              // main steps: slot = step % 3 == tap % 3 (9 taps per chunk)
        read_w_frags<TERMS, WIMG>(f, wring + slot * WBUF + kq * COUTP + wn * NT * 16 + li);
    };
    auto read_x = [&](Frags& f, int tap) {
        const int kh = tap / 3, kw = tap - kh * 3;
        const int toff = DG2 ? (kh == 2 ? IW : 0) + (kw == 2 ? 1 : 0) : kh * IW + kw;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            f.xh[t] = tile[kq * PL + pbase[t] + toff];
            if (TERMS == 3) f.xl[t] = tile[(4 + kq) * PL + pbase[t] + toff];
        }
    };
    static_assert(MT % 2 == 0, "a step's MFMAs are issued as two halves (pixel tiles)");
    auto mfma_half = [&](const Frags& f, int half, int tap) {
        const int ph = DG2 ? (tap / 3 != 1 ? 2 : 0) + (tap % 3 != 1 ? 1 : 0) : 0;      // (py, px): a centre row / column tap lands on even rows / columns
#pragma unroll
        for (int t = half * (MT / 2); t < (half + 1) * (MT / 2); ++t)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[ph][t][n] = mfma_split<TERMS>(f.wh[n], f.wl[n], f.xh[t], f.xl[t], acc[ph][t][n]);
    };
    static_assert(WRING == 3, "schedule below assumes a 3-slot ring");
    // Schedule of step s (one tap of one 32-channel chunk), one barrier per step, placed between the two MFMA halves:
    //   issue copy W(s+2) -> slot (s+2)%3        (its previous content, W(s-1), was last read before the barrier of step s-1)
    //   read the pixel fragments of step s+1     (hidden under ...)
    //   MFMAs of step s, first half
    //   wait: W(s+1) landed [counted vmcnt: W(s+2) stays in flight], LDS reads so far complete; barrier
    //   read the weight fragments of step s+1    (hidden under ...)
    //   MFMAs of step s, second half
    // so a weight copy has 1.5 steps of MFMAs to hide under and the fragment reads half a step.
    auto mid_sync = [&](bool copy_in_flight) {
        if constexpr (COUNTED) {
            __builtin_amdgcn_sched_barrier(0);  // keep the first-half MFMAs in front of the wait (the scheduler would sink them)
            if (copy_in_flight) wait_vmcnt_imm<GW>(); else wait_vmcnt_imm<0>();
            wait_lgkmcnt0();
            wg_barrier();
        } else {
            __syncthreads();
        }
    };
    Frags fr[2];
    if constexpr (SCC > 0) {
        // shortcut pre-phase: chunk c's 1x1 weights wait in ring slot 2 - c, step 0's 3x3 weights and the first halo chunk are in flight throughout
#pragma unroll
        for (int c = 0; c < SCC; ++c) issue_rows(a.sc_whi, a.sc_wlo, c * 4, 2 - c);
        issue_weights(0, 0);
        if (SCC == 1) issue_weights(1, 1);
        // staging roles: output pixel p of the TH x 32 tile, channel octet oc (8 consecutive lanes = 8 consecutive pixels of one octet)
        constexpr int SNIT = TH * 128 / 256;
        static_assert(SNIT * 256 == TH * 128, "shortcut staging deals whole iterations");
        int sgoff[SNIT], sslot[SNIT];
#pragma unroll
        for (int it = 0; it < SNIT; ++it) {
            const int idx = tid + it * 256;
            const int p = stage_pixel(idx), oc = stage_octet(idx);
            const int r = p >> 5, col = p & 31, oy = oy0 + r, ox = ox0 + col;
            // oy < Ho = (sc_H - 1) / sc_S + 1  =>  sc_S * oy <= sc_H - 1: a valid output pixel's source pixel is inside the block input
            sgoff[it] = (oy < a.Ho && ox < a.Wo) ? (oy * a.sc_S * a.sc_W + ox * a.sc_S) * (SCC * 32) + oc * 8 : -1;
            sslot[it] = oc * PL + (r + 1) * IW + col + 1;
        }
        const float* __restrict__ sxb = a.sc_x + (size_t)b * a.sc_H * a.sc_W * (SCC * 32);
        f4 sv[SNIT][2];
        auto load_sc = [&](int c) {
#pragma unroll
            for (int it = 0; it < SNIT; ++it) {
                sv[it][0] = sv[it][1] = (f4){0.f, 0.f, 0.f, 0.f};
                if (sgoff[it] >= 0) {
                    const float* src = sxb + sgoff[it] + c * 32;
                    sv[it][0] = *reinterpret_cast<const f4*>(src);
                    sv[it][1] = *reinterpret_cast<const f4*>(src + 4);
                }
            }
        };
        load_sc(0);
        load_tile(0);
#pragma unroll
        for (int c = 0; c < SCC; ++c) {
#pragma unroll
            for (int it = 0; it < SNIT; ++it) {
                store_split<TERMS, PL>(tile, sslot[it], sv[it][0], sv[it][1]);
            }
            if (c + 1 < SCC) load_sc(c + 1);
            __syncthreads();                    // shortcut pixels visible; every copy issued so far has landed
            read_w(fr[0], 2 - c);
            read_x(fr[0], 4);                   // the centre tap's positions
            mfma_half(fr[0], 0, 4);
            mfma_half(fr[0], 1, 4);
            __syncthreads();                    // fragment reads done: the tile and the slot may be overwritten
        }
        if (SCC == 2) issue_weights(1, 1);
        // D * f: the epilogue's per-clip scale q turns it back into D * sd (f = sd / q), whatever the gate
        const float* __restrict__ fv = a.sc_vec + (size_t)b * a.cout;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const f4 fq = *reinterpret_cast<const f4*>(fv + c0 + (wn * NT + n) * 16 + kq * 4);
#pragma unroll
            for (int t = 0; t < MT; ++t) acc[0][t][n] = acc[0][t][n] * fq;
        }
    } else {
        issue_weights(0, 0);
        if (NSTEP > 1) issue_weights(1, 1);
        load_tile(0);
    }
#pragma unroll 1
    for (int chunk = 0; chunk < CIN / 32; ++chunk) {
        store_tile(chunk);                      // the tile is free: its last reads completed before the barrier of the previous tap 8
        if (COUNTED && chunk > 0) {              // W of this chunk's tap 0 landed at that barrier too; only W of tap 1 is in flight
            wait_vmcnt_imm<GW>();
            wait_lgkmcnt0();                    // tile writes visible
            wg_barrier();
        } else {
            __syncthreads();                    // tile visible; every weight copy issued so far has landed
        }
        if (chunk + 1 < CIN / 32) load_tile(chunk + 1);
        read_w(fr[0], 0);
        read_x(fr[0], tap_of(0));
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int step = chunk * 9 + tap;
            const bool more = step + 2 < NSTEP;
            if (more) issue_weights(step + 2, (tap + 2) % 3);
            mfma_half(fr[tap & 1], 0, tap);
            mid_sync(more);
            if (tap < 8) { read_w(fr[(tap + 1) & 1], (tap + 1) % 3); read_x(fr[(tap + 1) & 1], tap_of(tap + 1)); }
            mfma_half(fr[tap & 1], 1, tap);
        }
    }

    if constexpr (DG2) {
        // four phases: dx[2 * by + py][2 * bx + px] for the base pixel (by, bx) of the dy grid; the (even, even) phase also takes the gradient that
        // arrives on the dy grid (the stride-2 1x1 shortcut reads exactly those pixels of x)
        const size_t ohw = (size_t)a.Ho * a.Wo;
        float* __restrict__ yb = a.y + (size_t)b * ohw * a.cout;
        const float* __restrict__ rq = a.res_q ? a.res_q + (size_t)b * a.H * a.W * a.cout : nullptr;
#pragma unroll
        for (int ph = 0; ph < 4; ++ph) {
            const int py = ph >> 1, px = ph & 1;
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                const int id = wm * MT + t;
                const int by = oy0 + (id >> 1), bx = ox0 + (id & 1) * 16 + li;
                const int oy = 2 * by + py, ox = 2 * bx + px;
                if (by < a.H && bx < a.W && oy < a.Ho && ox < a.Wo) {
#pragma unroll
                    for (int n = 0; n < NT; ++n) {
                        const int co = (wn * NT + n) * 16 + kq * 4;
                        if (co < a.cout) {
                            f4 v = acc[ph][t][n];
                            if (ph == 0 && rq) v += *reinterpret_cast<const f4*>(rq + ((size_t)by * a.W + bx) * a.cout + co);
                            *reinterpret_cast<f4*>(yb + ((size_t)oy * a.Wo + ox) * a.cout + co) = v;
                        }
                    }
                }
            }
        }
        return;
    }

    // epilogue: v = acc + bias; relu; v*scale + shift.  Pixel offsets are 32-bit and computed once per pixel tile; the
    // per-image base is a scalar.  NHWC: one 16-byte store per (pixel tile, channel tile); NCHW (final_conv1 only): 4 stores.
    f4 gsum[NT], gsq[NT];
    int pixo[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int id = wm * MT + t;
        const int oy = oy0 + (id >> 1), ox = ox0 + (id & 1) * 16 + li;
        pixo[t] = (oy < a.Ho && ox < a.Wo) ? oy * a.Wo + ox : -1;
    }
    const int hw = a.Ho * a.Wo;
    float* __restrict__ yb = a.y + (size_t)b * hw * a.cout;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        gsum[n] = (f4){0.f, 0.f, 0.f, 0.f};
        gsq[n] = gsum[n];
        const int co = c0 + (wn * NT + n) * 16 + kq * 4;
        const f4 bi = a.bias ? *reinterpret_cast<const f4*>(a.bias + co) : (f4){0.f, 0.f, 0.f, 0.f};
        f4 sc = a.scale ? *reinterpret_cast<const f4*>(a.scale + co) : (f4){1.f, 1.f, 1.f, 1.f};
        f4 sh = a.shift ? *reinterpret_cast<const f4*>(a.shift + co) : (f4){0.f, 0.f, 0.f, 0.f};
        if constexpr (SCC > 0) {                // per-clip scale q and shift h (the launch passes no gate and no residual map, relu2 = 1)
            const float* __restrict__ qv = a.sc_vec + ((size_t)a.sc_B + b) * a.cout + co;
            sc = *reinterpret_cast<const f4*>(qv);
            sh = *reinterpret_cast<const f4*>(qv + (size_t)a.sc_B * a.cout);
        }
        const f4 gt = (a.gate && co < a.cout) ? *reinterpret_cast<const f4*>(a.gate + (size_t)b * a.cout + co) : (f4){1.f, 1.f, 1.f, 1.f};
        const bool rb = a.res != nullptr;
        const size_t rbase = (size_t)b * hw * a.cout;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            f4 v = acc[0][t][n] + bi;
            if (a.relu) v = relu4(v);
            v = v * sc + sh;
            if (a.gate) v = v * gt;
            if (rb && pixo[t] >= 0 && co < a.cout) v += residual_quad(a.res, a.res_bits, rbase + (size_t)pixo[t] * a.cout + co);
            if (a.relu2) v = relu4(v);
            if (pixo[t] >= 0) {
                if (!a.nchw) {
                    if (co < a.cout) *reinterpret_cast<f4*>(yb + pixo[t] * a.cout + co) = v;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (co + r < a.cout) yb[(co + r) * hw + pixo[t]] = v[r];
                }
                gsum[n] += v;
                if (a.gap2) gsq[n] += v * v;
            }
        }
    }
    if (a.gap) {            // no LDS reads follow the last step's barrier: the LDS is free for the reduction
        float* sred = reinterpret_cast<float*>(lds);        // [WM][COUTP] sums, then [WM][COUTP] sums of squares
#pragma unroll
        for (int n = 0; n < NT; ++n) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float s = gsum[n][r];
                s = row16_sum(s);
                if (li == 0) sred[wm * COUTP + (wn * NT + n) * 16 + kq * 4 + r] = s;
                if (a.gap2) {
                    float q = gsq[n][r];
                    q = row16_sum(q);
                    if (li == 0) sred[(WM + wm) * COUTP + (wn * NT + n) * 16 + kq * 4 + r] = q;
                }
            }
        }
        // LDS traffic only: wait for the scratch writes, not (as __syncthreads would) for the tile's output stores to be acknowledged by memory
        wait_lgkmcnt0();
        wg_barrier();
        if (tid < (SPLIT ? COUTP : a.cout)) {
            float s = 0.f;
#pragma unroll
            for (int m = 0; m < WM; ++m) s += sred[m * COUTP + tid];
            a.gap[((size_t)b * a.tiles + tile_id) * a.cout + c0 + tid] = s;
            if (a.gap2) {
                float q = 0.f;
#pragma unroll
                for (int m = 0; m < WM; ++m) q += sred[(WM + m) * COUTP + tid];
                a.gap2[((size_t)b * a.tiles + tile_id) * a.cout + c0 + tid] = q;
            }
        }
    }
}

// ---- stride-2 stage entries (32 -> 64, 64 -> 128) on parity planes ----------------------------------------------------------------
// Tap (kh, kw) of output pixel (oy, ox) reads input (2 oy + kh - 1, 2 ox + kw - 1).  By (row, column) parity the input splits into four planes and
// every tap reads exactly one of them at UNIT stride:
//   plane 0 (even, even): TH x 32 pixels, tap 4           plane 1 (even, odd): TH x 33, taps 3, 5
//   plane 2 (odd, even): (TH + 1) x 32, taps 1, 7         plane 3 (odd, odd): (TH + 1) x 33, taps 0, 2, 6, 8
// Plane pixel (pr, pc) of the tile at (oy0, ox0) is input (2 (oy0 + pr) - rp, 2 (ox0 + pc) - cp), rp / cp = 1 for the odd planes; inside its plane a
// tap reads (row + (kh == 2), col + (kw == 2)).  The interleaved form (conv3x3_bf16_kernel, S = 2) stages a (2 TH + 1) x 65 halo per 32-channel chunk,
// which caps it at 2-row tiles (41.6 KB); here the LDS tile holds ONE plane of one chunk at a time (TH = 8: 38 KB), so that the tiles can be 4 or 8 rows
// and a step has the body kernels' 48 MFMAs per wave.  The workgroup walks (chunk, plane) sub-chunks; the next plane's pixels are in flight in
// registers while the current plane's 1, 2 or 4 taps run; the weight ring streams the taps in plane order (s2p_tap) from the unchanged packed images
// with the schedule of conv3x3_bf16_kernel, plus one barrier per plane swap.  The four-tap plane comes last in a chunk: it covers the load of the next
// chunk's first plane.
// Pooling partials keep the interleaved form's layout (eg_conv3x3_gap_tiles: one per 2 x 32 output block): a wave's four pixel tiles ARE one such
// block for its channel range, so every wave writes its own sums and no cross-wave fold is needed.
// The launch function picks the form by the size of the launch (conv_s2_form), so the two forms must agree bit for bit (a clip's result may not
// depend on the batch it is computed in): the interleaved form accumulates its taps in the same order, and the partial is folded here as there,
// row sums first, then the two rows.
template <int TH> struct ConvGeomS2P {
    static constexpr int PW = 33;                       // row length of every plane's LDS image (the odd-column planes hold 33 columns)
    static constexpr int NPIX = (TH + 1) * PW;          // the largest plane, (odd, odd)
    static constexpr int PL = (NPIX + 15) / 16 * 16;
};

template <int CIN, int NTT, int TH, int WM, int WN, int TERMS, bool AFF>
__global__ __launch_bounds__(256, 2) void conv3x3_s2_planes_kernel(ConvArgs a, const bf8* __restrict__ whi, const bf8* __restrict__ wlo) {
    using G = ConvGeomS2P<TH>;
    constexpr int COUTP = NTT * 16, PW = G::PW, NPIX = G::NPIX, PL = G::PL;
    constexpr int MT = TH * 2 / WM, NT = NTT / WN;
    using L = RingLds<PL, COUTP, TERMS>;
    constexpr int NIMG = L::NIMG, TILE = L::TILE, WIMG = L::WIMG, WBUF = L::WBUF;
    constexpr int NSTEP = (CIN / 32) * 9;
    static_assert(WM * WN == 4 && MT == 4 && NT * WN == NTT, "a wave owns one 2 x 32 output block (four pixel tiles) of its channel range");
    extern __shared__ __attribute__((aligned(16))) bf8 lds[];      // RingLds: TILE + WRING * WBUF slots
    bf8* tile = lds;
    bf8* wring = lds + TILE;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, kq = lane >> 4;
    const int wm = wave / WN, wn = wave % WN;
    int tile_id = blockIdx.x, b = blockIdx.y;       // XCD-aware tile order, as conv3x3_bf16_kernel
    {
        const int total = gridDim.x * gridDim.y;
        if ((total & 7) == 0) {
            const int lin = blockIdx.y * gridDim.x + blockIdx.x;
            const int log = (lin & 7) * (total >> 3) + (lin >> 3);
            b = log / (int)gridDim.x;
            tile_id = log - b * (int)gridDim.x;
        }
    }
    const int ty = tile_id / a.tiles_x, tx = tile_id - ty * a.tiles_x;
    const int oy0 = ty * TH, ox0 = tx * 32;

    int pbase[MT];                                  // pixel tile t of the wave: output row 2 wm + (t >> 1), columns (t & 1) * 16 ..
#pragma unroll
    for (int t = 0; t < MT; ++t) pbase[t] = (2 * wm + (t >> 1)) * PW + (t & 1) * 16 + li;
    f4 acc[MT][NT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[t][n] = (f4){0.f, 0.f, 0.f, 0.f};
    const float* xb = a.x + (size_t)b * a.H * a.W * CIN;

    // one step's weights = NIMG runs of WIMG slots; 64-slot (1 KiB) pieces dealt round-robin to the 4 waves, the same count for every wave
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    constexpr int PIECES = WIMG / 64;
    static_assert(PIECES % 4 == 0, "every wave copies PIECES / 4 pieces of each image (the per-step wait is a counted vmcnt)");
    constexpr int GW = NIMG * PIECES / 4;
    const unsigned lane_b = lane * (unsigned)sizeof(bf8);
    auto issue_weights = [&](int step, int buf) {   // chunk-major steps, the chunk's taps in plane order
        const int chunk = step / 9, tap = s2p_tap(step - chunk * 9);
        const size_t gbase = (size_t)(tap * (CIN / 8) + chunk * 4) * COUTP;
#pragma unroll
        for (int img = 0; img < NIMG; ++img) {
            const bf8* src = (img ? wlo : whi) + gbase;
#pragma unroll
            for (int p = 0; p < PIECES / 4; ++p) {
                const int piece = p * 4 + wave_u;
                // a uniform base and a 32-bit lane offset: one address register for every copy of the kernel
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(reinterpret_cast<const char*>(src + piece * 64) + lane_b),
                                                 (__attribute__((address_space(3))) void*)(wring + buf * WBUF + img * WIMG + piece * 64), 16, 0, 0);
            }
        }
    };
    // plane staging: one lane = one plane pixel x 8 channels per iteration.  The roles are the same for every plane and chunk: the element offset of
    // the (even, even) pixel of the lane's position (plane (rp, cp) reads rp rows and cp columns before it), the LDS slot, and one bit per plane:
    // the position belongs to the plane and lies inside the image.  Loads and stores are unconditional (no divergent branches, and a fixed number
    // of loads per plane for the counted waits of the schedule): a position outside the plane or the image reads the clip's first pixel and is
    // stored as zero (the padding); positions past the largest plane share the image's last slot, which no tap reads.
    constexpr int NIT = (((NPIX + 7) / 8) * 32 + 255) / 256;
    constexpr int LV = 2 * NIT;                     // global loads of one plane per lane
    static_assert(PL > NPIX, "the spare slot");
    f4 pv[NIT][2];
    int goff[NIT], pmask = 0;                       // bit it * 4 + pl
    static_assert(NIT * 4 <= 32, "one mask word");
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int idx = tid + it * 256;
        const int p = stage_pixel(idx), oc = stage_octet(idx);
        const int pr = p / PW, pc = p - pr * PW;
        const int gy0 = 2 * (oy0 + pr), gx0 = 2 * (ox0 + pc);
        goff[it] = (gy0 * a.W + gx0) * CIN + oc * 8;
#pragma unroll
        for (int pl = 0; pl < 4; ++pl) {
            const int rp = pl >> 1, cp = pl & 1, gy = gy0 - rp, gx = gx0 - cp;
            if (p < NPIX && pr < TH + rp && pc < 32 + cp && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) pmask |= 1 << (it * 4 + pl);
        }
    }
    auto load_plane = [&](int chunk, int pl) {
        const int poff = ((pl >> 1) * a.W + (pl & 1)) * CIN - chunk * 32;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const float* src = xb + (((pmask >> (it * 4 + pl)) & 1) ? goff[it] - poff : 0);
            pv[it][0] = *reinterpret_cast<const f4*>(src);
            pv[it][1] = *reinterpret_cast<const f4*>(src + 4);
        }
    };
    const int ocs = (tid >> 3) & 3, oc8s = ocs * 8, p0 = (tid >> 5) * 8 + (tid & 7);        // this lane's channel octet and first position
    auto store_plane = [&](int chunk, int pl) {
        // AFF: the input affine of the training path, x' = x * in_scale[ci] + in_shift[ci] inside the image (these loads are the youngest memory
        // operations when they are used: the wait for them lands every copy in flight, which the counted waits tolerate -- they only assume that
        // no FEWER operations were issued)
        f4 s0, s1, h0, h1;
        if constexpr (AFF) {
            s0 = *reinterpret_cast<const f4*>(a.in_scale + chunk * 32 + oc8s); s1 = *reinterpret_cast<const f4*>(a.in_scale + chunk * 32 + oc8s + 4);
            h0 = *reinterpret_cast<const f4*>(a.in_shift + chunk * 32 + oc8s); h1 = *reinterpret_cast<const f4*>(a.in_shift + chunk * 32 + oc8s + 4);
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            // zeroed by a bit mask, not a select: a select becomes a divergent branch around the multiply-adds, and the memory waits behind a
            // branch are no longer counted
            const u32x4_t m = (u32x4_t)(0u - (unsigned)((pmask >> (it * 4 + pl)) & 1));
            f4 x0 = pv[it][0], x1 = pv[it][1];
            if constexpr (AFF) { x0 = x0 * s0 + h0; x1 = x1 * s1 + h1; }
            const f4 v0 = __builtin_bit_cast(f4, __builtin_bit_cast(u32x4_t, x0) & m), v1 = __builtin_bit_cast(f4, __builtin_bit_cast(u32x4_t, x1) & m);
            bf8 hi, lo;
            split_octet<TERMS == 3>(v0, v1, hi, lo);
            const int p = p0 + it * 64, slot = ocs * PL + (p < PL - 1 ? p : PL - 1);
            tile[slot] = hi;
            if (TERMS == 3) tile[4 * PL + slot] = lo;
        }
    };

    using Frags = ConvFrags<NT, MT>;
    auto read_w = [&](Frags& f, int slot) { read_w_frags<TERMS, WIMG>(f, wring + slot * WBUF + kq * COUTP + wn * NT * 16 + li); };
    auto read_x = [&](Frags& f, int tap) {          // unit stride inside the tap's plane
        const int toff = (tap / 3 == 2 ? PW : 0) + (tap % 3 == 2 ? 1 : 0);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            f.xh[t] = tile[kq * PL + pbase[t] + toff];
            if (TERMS == 3) f.xl[t] = tile[(4 + kq) * PL + pbase[t] + toff];
        }
    };
    auto mfma_half = [&](const Frags& f, int half) {
#pragma unroll
        for (int t = half * (MT / 2); t < (half + 1) * (MT / 2); ++t)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[t][n] = mfma_split<TERMS>(f.wh[n], f.wl[n], f.xh[t], f.xl[t], acc[t][n]);
    };
    // Schedule.  Step s = (chunk, k) runs tap s2p_tap(k); W(s) = its weights, in ring slot k % 3.  As in conv3x3_bf16_kernel a step is
    //   [issue W(s+2)]  MFMAs first half  wait: W(s+1) landed; barrier  read the fragments of s+1  MFMAs second half
    // and a step that ends its plane (k = 0, 2, 4, and 8 when a chunk follows) SWAPS after that barrier instead:
    //   store the next plane (its pixels are in registers)  MFMAs second half  barrier  issue W(s+3)  load the plane after the next  fragments of s+1
    // The memory counter retires in order, and the mid-step wait is "all but the youngest N operations": a plane's LV loads are issued BEHIND
    // W(s+3), which the step after the swap would otherwise issue, so they stay in flight through the waits of the next two steps (N = GW + LV:
    // the loads and one weight copy) and are forced to land only by the third -- or by the next swap's store.  The waits per k (L = the plane
    // load issued at the last swap, none after k = 4 of the last chunk):
    //   k = 0, 1, 3, 5 (after a swap; W(s+2) was issued there): younger than W(s+1) are W(s+2), L      -> GW + LV
    //   k = 2, 4, 6    (second step; issues W(s+2)):            younger than W(s+1) are L, W(s+2)      -> GW + LV
    //   k = 7, 8       (issue W(s+2) while a chunk follows):    younger than W(s+1) is W(s+2)          -> GW, or 0 in the last chunk
    auto mid_sync = [&](int k, bool nxt) {
        __builtin_amdgcn_sched_barrier(0);          // keep the first-half MFMAs in front of the wait (the scheduler would sink them)
        if (k <= 4) wait_vmcnt_imm<GW + LV>();
        else if (k <= 6) { if (nxt) wait_vmcnt_imm<GW + LV>(); else wait_vmcnt_imm<GW>(); }
        else { if (nxt) wait_vmcnt_imm<GW>(); else wait_vmcnt_imm<0>(); }
        wait_lgkmcnt0();
        wg_barrier();
    };
    Frags fr[2];
    issue_weights(0, 0);
    issue_weights(1, 1);
    load_plane(0, 0);
    store_plane(0, 0);
    wait_vmcnt_imm<0>();
    wait_lgkmcnt0();
    wg_barrier();
    issue_weights(2, 2);
    __builtin_amdgcn_sched_barrier(0);
    load_plane(0, 1);
    read_w(fr[0], 0);
    read_x(fr[0], s2p_tap(0));
#pragma unroll 1
    for (int chunk = 0; chunk < CIN / 32; ++chunk) {
        // opaque to the optimiser per chunk: hoisted out of the loop, the masks (one vector per plane and iteration) and the copies' per-chunk
        // addresses cost more registers than the kernel has
        int chunk_u = chunk;
        asm volatile("" : "+s"(chunk_u), "+v"(pmask));
        const bool nxt = chunk_u + 1 < CIN / 32;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int step = chunk_u * 9 + k;
            const bool after_swap = k == 0 || k == 1 || k == 3 || k == 5;
            const bool swap = k == 0 || k == 2 || k == 4 || (k == 8 && nxt);
            const int kn = (k + 1) % 9, fn = k < 8 ? (k + 1) & 1 : 0;           // the next step's k and fragment set (a chunk starts on set 0)
            if (!after_swap && step + 2 < NSTEP) issue_weights(step + 2, (k + 2) % 3);
            mfma_half(fr[k & 1], 0);
            mid_sync(k, nxt);
            if (swap) {
                // every wave holds this step's fragments: the tile takes the next plane, under the second half of the MFMAs
                store_plane(k < 8 ? chunk_u : chunk_u + 1, s2p_plane(kn));
                mfma_half(fr[k & 1], 1);
                wait_lgkmcnt0();
                wg_barrier();
                issue_weights(step + 3, k % 3);     // slot (k + 3) % 3: W(s) was last read before this step's first barrier
                __builtin_amdgcn_sched_barrier(0);  // the loads stay behind the weight copy
                if (k == 0) load_plane(chunk_u, 2);
                else if (k == 2) load_plane(chunk_u, 3);
                else if (k == 8) load_plane(chunk_u + 1, 1);
                else if (nxt) load_plane(chunk_u + 1, 0);
                read_w(fr[fn], kn % 3);
                read_x(fr[fn], s2p_tap(kn));
            } else {
                if (k < 8) { read_w(fr[fn], kn % 3); read_x(fr[fn], s2p_tap(kn)); }
                mfma_half(fr[k & 1], 1);
            }
        }
    }

    // epilogue: v = acc + bias; relu; v * scale + shift; one 16-byte NHWC store per (pixel tile, channel tile)
    int pixo[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int oy = oy0 + 2 * wm + (t >> 1), ox = ox0 + (t & 1) * 16 + li;
        pixo[t] = (oy < a.Ho && ox < a.Wo) ? oy * a.Wo + ox : -1;
    }
    const int hw = a.Ho * a.Wo;
    float* __restrict__ yb = a.y + (size_t)b * hw * COUTP;
    // the wave's 2 x 32 block in the numbering of eg_conv3x3_gap_tiles (2-row tiles); a block below the map's last row does not exist
    const bool blk_ok = oy0 + 2 * wm < a.Ho;
    const size_t gbase = ((size_t)b * a.tiles + (size_t)(ty * (TH / 2) + wm) * a.tiles_x + tx) * COUTP;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        f4 gsum[2], gsq[2];                         // per output row of the block: the interleaved form's summation order (a wave per row, then the two rows)
        gsum[0] = gsum[1] = gsq[0] = gsq[1] = (f4){0.f, 0.f, 0.f, 0.f};
        const int co = (wn * NT + n) * 16 + kq * 4;
        const f4 bi = a.bias ? *reinterpret_cast<const f4*>(a.bias + co) : (f4){0.f, 0.f, 0.f, 0.f};
        const f4 sc = a.scale ? *reinterpret_cast<const f4*>(a.scale + co) : (f4){1.f, 1.f, 1.f, 1.f};
        const f4 sh = a.shift ? *reinterpret_cast<const f4*>(a.shift + co) : (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            f4 v = acc[t][n] + bi;
            if (a.relu) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            }
            v = v * sc + sh;
            if (pixo[t] >= 0) {
                *reinterpret_cast<f4*>(yb + pixo[t] * COUTP + co) = v;
                gsum[t >> 1] += v;
                if (a.gap2) gsq[t >> 1] += v * v;
            }
        }
        if (a.gap) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                gsum[0][r] = (0.f + row16_sum(gsum[0][r])) + row16_sum(gsum[1][r]);
                if (a.gap2) gsq[0][r] = (0.f + row16_sum(gsq[0][r])) + row16_sum(gsq[1][r]);
            }
            if (li == 0 && blk_ok) {
                *reinterpret_cast<f4*>(a.gap + gbase + co) = gsum[0];
                if (a.gap2) *reinterpret_cast<f4*>(a.gap2 + gbase + co) = gsq[0];
            }
        }
    }
}

// ---- 32 -> 32 channels, stride 1: persistent variant (the HBM-bound first stage) -------------------------------------------------
// The tiled kernel above gives a 32-channel workgroup 108 MFMAs per wave between a cold halo load and its stores: its lifetime is
// almost all memory latency, hidden only by co-resident workgroups (3.3-3.8 TB/s).  Here a workgroup walks a run of consecutive
// 4 x 32-pixel tiles: all 9 taps' weights (36 KB of hi/lo images) are copied to LDS once, the NEXT tile's halo pixels (and this tile's
// residual, for the fused SE tail) are in flight in registers while the 9 taps of the current tile run, and the taps need no barrier
// (weights and tile are static): two barriers per tile instead of ten.  Same arithmetic and summation order as the tiled kernel.
constexpr int C32_ROWS = 4;     // tile height of the walk (8-row tiles were measured and retired: tools/experiments/README.md)
// its LDS, in bf8 slots: [tile][hi image: 9 taps x 4 octet rows x 32 channels][lo image], then the pooling scratch in floats
template <int TERMS> struct C32Lds {
    static constexpr int NIMG = (TERMS == 3) ? 2 : 1;
    static constexpr int TILE = NIMG * 4 * ConvGeom<1, C32_ROWS>::PL, WTAP = 4 * 32, WIMG = 9 * WTAP;
    static constexpr size_t BYTES = sizeof(bf8) * (size_t)(TILE + NIMG * WIMG) + 2 * 4 * 32 * sizeof(float);        // + [4 waves][32] sums, then the squares
};
template <int TERMS>
__global__ __launch_bounds__(256, 2) void conv3x3_c32_persistent_kernel(ConvArgs a, const bf8* __restrict__ whi, const bf8* __restrict__ wlo,
                                                                     int total_tiles) {
    constexpr int TH = C32_ROWS;
    using G = ConvGeom<1, TH>;
    using L = C32Lds<TERMS>;
    constexpr int CIN = 32, IW = G::IW, NPIX = G::NPIX, PL = G::PL, MT = TH / 2, NT = 2;
    constexpr int NIMG = L::NIMG, TILE = L::TILE, WTAP = L::WTAP, WIMG = L::WIMG;
    extern __shared__ __attribute__((aligned(16))) bf8 lds[];      // tile | weights (hi [tap][octet][co], lo) | gap scratch
    bf8* tile = lds;
    bf8* wl = lds + TILE;
    float* sred = reinterpret_cast<float*>(lds + TILE + NIMG * WIMG);      // gap scratch [4 waves][32 floats], then the same again for the sums of squares

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, kq = lane >> 4;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    // XCD-aware: workgroups are dealt round-robin to the 8 XCDs; XCD k walks a contiguous eighth of the tile list
    int wg = blockIdx.x;
    if ((gridDim.x & 7) == 0) wg = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    // Walk order: workgroup w takes tiles w, w + G, w + 2G, ... (G = grid size), so that at any moment the G resident workgroups work on G
    // CONSECUTIVE tiles (each XCD on a contiguous run of G / 8): the halo rows shared by vertically adjacent tiles are fetched by neighbours at
    // about the same time and hit in that XCD's L2.  (A contiguous run per workgroup re-read them from memory 4 tiles later: 260 MB read per
    // launch at the memory-side counters against 196 MB for the tiled kernel.)
    const int NWG = gridDim.x;
    const int t_begin = wg, t_end = total_tiles;
    if (t_begin >= t_end) return;

    // all weights -> LDS, once: NIMG x 18 pieces of 64 slots, dealt round-robin to the 4 waves
#pragma unroll
    for (int img = 0; img < NIMG; ++img) {
        const bf8* src = img ? wlo : whi;
#pragma unroll
        for (int p = 0; p < 5; ++p) {
            const int piece = p * 4 + wave_u;
            if (piece < WIMG / 64)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + piece * 64 + lane),
                                                 (__attribute__((address_space(3))) void*)(wl + img * WIMG + piece * 64), 16, 0, 0);
        }
    }

    // staging roles (tile independent): pixel p of the 6 x 34 halo tile, channel octet oc
    constexpr int NIT = (((NPIX + 7) / 8) * 32 + 255) / 256;
    int piy[NIT], pix[NIT], lslot[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int idx = tid + it * 256;
        const int p = stage_pixel(idx), oc = stage_octet(idx);
        piy[it] = p / IW;
        pix[it] = p - piy[it] * IW;
        lslot[it] = p < NPIX ? oc * PL + p : -1;
    }
    const int oc8 = ((tid >> 3) & 3) * 8;
    f4 isc[2] = {(f4){1.f, 1.f, 1.f, 1.f}, (f4){1.f, 1.f, 1.f, 1.f}}, ish[2] = {(f4){0.f, 0.f, 0.f, 0.f}, (f4){0.f, 0.f, 0.f, 0.f}};
    if (a.in_scale) {
        isc[0] = *reinterpret_cast<const f4*>(a.in_scale + oc8); isc[1] = *reinterpret_cast<const f4*>(a.in_scale + oc8 + 4);
        ish[0] = *reinterpret_cast<const f4*>(a.in_shift + oc8); ish[1] = *reinterpret_cast<const f4*>(a.in_shift + oc8 + 4);
    }
    f4 pv[NIT][2];
    // tile coordinates advance incrementally along the walk (an integer division per use costs ~30 VALU instructions; this kernel
    // issues 4 non-MFMA VALU instructions per MFMA as it is: profiles/r02k_pmc_conv32_persistent.txt)
    struct Coord { int b, ty, tx; };
    const int tiles_y = a.tiles / a.tiles_x;
    const int adv_b = NWG / a.tiles, adv_r = NWG - adv_b * a.tiles, adv_ty = adv_r / a.tiles_x, adv_tx = adv_r - adv_ty * a.tiles_x;
    auto advance = [&](Coord& c) {                // + NWG tiles, without a division
        c.tx += adv_tx;
        if (c.tx >= a.tiles_x) { c.tx -= a.tiles_x; ++c.ty; }
        c.ty += adv_ty;
        if (c.ty >= tiles_y) { c.ty -= tiles_y; ++c.b; }
        c.b += adv_b;
    };
    auto load_tile = [&](const Coord& c) {
        const int b = c.b;
        const int iy0 = c.ty * TH - 1, ix0 = c.tx * 32 - 1;
        const float* __restrict__ xb = a.x + (size_t)b * a.H * a.W * CIN;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            pv[it][0] = pv[it][1] = (f4){0.f, 0.f, 0.f, 0.f};
            const int gy = iy0 + piy[it], gx = ix0 + pix[it];
            if (lslot[it] >= 0 && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
                const float* src = xb + (gy * a.W + gx) * CIN + oc8;
                pv[it][0] = *reinterpret_cast<const f4*>(src);
                pv[it][1] = *reinterpret_cast<const f4*>(src + 4);
                if (a.in_scale) {                   // the BatchNorm in front of this convolution, folded into the staging (in-image pixels only)
                    pv[it][0] = pv[it][0] * isc[0] + ish[0];
                    pv[it][1] = pv[it][1] * isc[1] + ish[1];
                }
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (lslot[it] >= 0) {
                store_split<TERMS, PL>(tile, lslot[it], pv[it][0], pv[it][1]);
            }
        }
    };
    int pbase[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int id = wave * MT + t;
        pbase[t] = (id >> 1) * IW + (id & 1) * 16 + li;
    }
    // (Keeping the hi weight fragments of all 9 taps in registers -- 72 VGPRs, a quarter less LDS fragment traffic -- measured no faster
    //  in the step and 7 % slower alone: the fragment reads are not what bounds this kernel.)
    using Frags = ConvFrags<NT, MT>;
    auto read_frags = [&](Frags& f, int tap) {
        const int kh = tap / 3, kw = tap - kh * 3, toff = kh * IW + kw;
        read_w_frags<TERMS, WIMG>(f, wl + tap * WTAP + kq * 32 + li);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            f.xh[t] = tile[kq * PL + pbase[t] + toff];
            if (TERMS == 3) f.xl[t] = tile[(4 + kq) * PL + pbase[t] + toff];
        }
    };

    const int hw = a.Ho * a.Wo;
    // channel-wise epilogue constants of this lane's 2 x 4 output channels
    f4 bi[NT], sc[NT], sh[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int co = n * 16 + kq * 4;
        bi[n] = a.bias ? *reinterpret_cast<const f4*>(a.bias + co) : (f4){0.f, 0.f, 0.f, 0.f};
        sc[n] = a.scale ? *reinterpret_cast<const f4*>(a.scale + co) : (f4){1.f, 1.f, 1.f, 1.f};
        sh[n] = a.shift ? *reinterpret_cast<const f4*>(a.shift + co) : (f4){0.f, 0.f, 0.f, 0.f};
    }

    f4 rsn[MT][NT];
    auto load_res = [&](const Coord& c) {
        const int ty = c.ty, tx = c.tx;
        const size_t rbase = (size_t)c.b * hw * 32;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int id = wave * MT + t;
            const int oy = ty * TH + (id >> 1), ox = tx * 32 + (id & 1) * 16 + li;
            const bool ok = a.res && oy < a.Ho && ox < a.Wo;
#pragma unroll
            for (int n = 0; n < NT; ++n)
                rsn[t][n] = ok ? residual_quad(a.res, a.res_bits, rbase + (size_t)(oy * a.Wo + ox) * 32 + n * 16 + kq * 4) : (f4){0.f, 0.f, 0.f, 0.f};
        }
    };
    Coord cur;
    cur.b = t_begin / a.tiles;
    cur.ty = (t_begin - cur.b * a.tiles) / a.tiles_x;
    cur.tx = t_begin - cur.b * a.tiles - cur.ty * a.tiles_x;
    Coord nxt = cur;
    load_tile(cur);
    load_res(cur);
    wait_vmcnt_imm<0>();                       // the weight copies have landed (this wave's); the barrier below publishes all of them
    for (int L = t_begin; L < t_end; L += NWG, cur = nxt) {
        const int b = cur.b, tile_id = cur.ty * a.tiles_x + cur.tx;
        const int oy0 = cur.ty * TH, ox0 = cur.tx * 32;
        advance(nxt);
        store_tile();
        __syncthreads();                        // tile (and, first time, weights) visible
        // halo AND residual of the NEXT tile: in flight during this tile's 9 taps and epilogue
        int pixo[MT];
        f4 rs[MT][NT];
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int id = wave * MT + t;
            const int oy = oy0 + (id >> 1), ox = ox0 + (id & 1) * 16 + li;
            pixo[t] = (oy < a.Ho && ox < a.Wo) ? oy * a.Wo + ox : -1;
#pragma unroll
            for (int n = 0; n < NT; ++n) rs[t][n] = rsn[t][n];
        }
        const bool has_res = a.res != nullptr;
        if (L + NWG < t_end) load_res(nxt);
        if (L + NWG < t_end) load_tile(nxt);

        f4 acc[MT][NT];
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[t][n] = (f4){0.f, 0.f, 0.f, 0.f};
        Frags fr[2];
        read_frags(fr[0], 0);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            if (tap < 8) read_frags(fr[(tap + 1) & 1], tap + 1);
            const Frags& f = fr[tap & 1];
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[t][n] = mfma_split<TERMS>(f.wh[n], f.wl[n], f.xh[t], f.xl[t], acc[t][n]);
        }

        float* __restrict__ yb = a.y + (size_t)b * hw * 32;
        f4 gsum[NT], gsq[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            gsum[n] = (f4){0.f, 0.f, 0.f, 0.f};
            gsq[n] = gsum[n];
            const int co = n * 16 + kq * 4;
            const f4 gt = a.gate ? *reinterpret_cast<const f4*>(a.gate + (size_t)b * 32 + co) : (f4){1.f, 1.f, 1.f, 1.f};
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                f4 v = acc[t][n] + bi[n];
                if (a.relu) v = relu4(v);
                v = v * sc[n] + sh[n];
                if (a.gate) v = v * gt;
                if (has_res && pixo[t] >= 0) v += rs[t][n];
                if (a.relu2) v = relu4(v);
                if (pixo[t] >= 0) {
                    *reinterpret_cast<f4*>(yb + pixo[t] * 32 + co) = v;
                    gsum[n] += v;
                    if (a.gap2) gsq[n] += v * v;
                }
            }
        }
        if (a.gap) {
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float sm = gsum[n][r];
                    sm = row16_sum(sm);
                    if (li == 0) sred[wave * 32 + n * 16 + kq * 4 + r] = sm;
                    if (a.gap2) {               // the squares' scratch follows the sums'
                        float q = gsq[n][r];
                        q = row16_sum(q);
                        if (li == 0) sred[128 + wave * 32 + n * 16 + kq * 4 + r] = q;
                    }
                }
        }
        __syncthreads();                        // every wave is done with the tile image (and the gap scratch is complete)
        if (a.gap && tid < 32) {
            float sm = 0.f;
#pragma unroll
            for (int m = 0; m < 4; ++m) sm += sred[m * 32 + tid];
            a.gap[((size_t)b * a.tiles + tile_id) * 32 + tid] = sm;
            if (a.gap2) a.gap2[((size_t)b * a.tiles + tile_id) * 32 + tid] = (sred[128 + tid] + sred[160 + tid]) + (sred[192 + tid] + sred[224 + tid]);
        }
    }
}

// ---- stem: Conv2d(1->C, 3x3, bias) -> ReLU -> BN, x [B,H,W] -> y NHWC ----------------------------
__global__ __launch_bounds__(256) void stem_conv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, float* __restrict__ y,
                                                        int B, int H, int W, int C) {
    // One workgroup per output row: the three input rows (zero padded) are staged in LDS once, thread = (pixel, channel quad) with the
    // quad fixed per thread (its 9 taps + bias + BN affine stay in registers), pixels strided by 256 / (C/4).  No per-element index
    // division (the first version spent four 64-bit divisions per output quad: 27 M VALU instructions per launch, VALU bound at 53 us).
    extern __shared__ float rows[];                     // [3][W + 2]
    const int cq_n = C >> 2, tid = threadIdx.x;
    const int b = blockIdx.x / H, oy = blockIdx.x - b * H, WP = W + 2;
    const float* xb = x + (size_t)b * H * W;
    for (int i = tid; i < 3 * WP; i += 256) {
        const int r = i / WP, c = i - r * WP, gy = oy + r - 1, gx = c - 1;
        rows[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? xb[gy * W + gx] : 0.f;
    }
    const int cq = tid % cq_n, px0 = tid / cq_n, pstep = 256 / cq_n;
    f4 wv[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wv[t] = *reinterpret_cast<const f4*>(w + t * C + cq * 4);
    const f4 bi = *reinterpret_cast<const f4*>(bias + cq * 4);
    const f4 sc = *reinterpret_cast<const f4*>(scale + cq * 4), sh = *reinterpret_cast<const f4*>(shift + cq * 4);
    __syncthreads();
    float* yrow = y + ((size_t)b * H + oy) * W * C + cq * 4;
    for (int ox = px0; ox < W; ox += pstep) {
        f4 acc = bi;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) acc += wv[kh * 3 + kw] * rows[kh * WP + ox + kw];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = fmaxf(acc[r], 0.f);
        *reinterpret_cast<f4*>(yrow + (size_t)ox * C) = acc * sc + sh;
    }
}

// ---- SE gate: GAP finish + FC -> ReLU -> FC -> sigmoid, one workgroup per clip ---------------------
__global__ __launch_bounds__(256) void se_gate_kernel(const float* __restrict__ gap, int tiles, const float* __restrict__ w1,
                                                      const float* __restrict__ b1, const float* __restrict__ w2,
                                                      const float* __restrict__ b2, float* __restrict__ gate, int C, float inv_hw) {
    __shared__ float m[256];
    __shared__ float h[32];
    const int b = blockIdx.x, t = threadIdx.x, R = C >> 3;
    {   // fixed-order (deterministic) two-level sum of the per-tile partials: blockDim/C groups x C channels
        const int c = t % C, g = t / C, G = blockDim.x / C;
        float s = 0.f;
        for (int i = g; i < tiles; i += G) s += gap[((size_t)b * tiles + i) * C + c];
        m[t] = s;
        __syncthreads();
        float tot = 0.f;
        if (t < C)
            for (int j = 0; j < G; ++j) tot += m[j * C + t];
        __syncthreads();
        if (t < C) m[t] = tot * inv_hw;
    }
    __syncthreads();
    if (t < R) {
        float s = b1[t];
        for (int c = 0; c < C; ++c) s += w1[t * C + c] * m[c];
        h[t] = fmaxf(s, 0.f);
    }
    __syncthreads();
    if (t < C) {
        float s = b2[t];
        for (int j = 0; j < R; ++j) s += w2[t * R + j] * h[j];
        gate[(size_t)b * C + t] = 1.f / (1.f + expf(-s));
    }
}

// ---- SE gate computed BEFORE conv2 runs ("gate from the input's moments") ------------------------------------------------------
// gate = sigmoid(W2 relu(W1 mean_hw(y) + b1) + b2), y = BN2(conv2(t1)) (ResNetBlocks.py:28-30,92-96).  The spatial mean of a 3x3 / pad 1 /
// stride 1 convolution is linear in shifted-window sums of its INPUT:
//     mean_hw(conv2(t1))[co] = 1/HW * sum_{tap, ci} W[co][ci][tap] * S[tap][ci],   S[(kh,kw)][ci] = sum of t1[.., ci] over the rows / columns
//     the tap reaches: everything, minus the last (kh = 0) or first (kh = 2) row, minus the last (kw = 0) or first (kw = 2) column, plus
//     the doubly removed corner.
// The total comes from conv1's per-tile channel sums (its `gap` output), the four border lines and corners are read from t1 itself.
// With the gate known up front, conv2's epilogue applies relu(y * gate + x) directly: the block's y tensor is never written and the
// separate tail pass (2 reads + 1 write of the activation) disappears.  One workgroup per clip; fixed-order sums (deterministic).
constexpr int GP_T = 1024;      // threads per clip: G = 1024 / C thread groups share every sum (many loads in flight: the kernel is latency bound)
__global__ __launch_bounds__(GP_T) void se_gate_pre_kernel(const float* __restrict__ t1, const float* __restrict__ gap, int tiles,
                                                           const float* __restrict__ w2img, const float* __restrict__ scale2,
                                                           const float* __restrict__ shift2, const float* __restrict__ w1, const float* __restrict__ b1,
                                                           const float* __restrict__ wf2, const float* __restrict__ bf2, float* __restrict__ gate,
                                                           int H, int W, int C, const float* __restrict__ ds_scale, const float* __restrict__ ds_shift,
                                                           float* __restrict__ sc_vec) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.x, t = threadIdx.x, G = GP_T / C, c = t % C, g = t / C, R = C >> 3;
    float* part = sm;                   // [5][GP_T]: total, first row, last row, first column, last column (per thread)
    float* S = sm + 5 * GP_T;           // [9][C]
    float* zp = S + 9 * C;              // [G][C]
    float* m = zp + GP_T;               // [C]
    float* hbuf = m + C;                // [R]
    const float* tb = t1 + (size_t)b * H * W * C;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll 4
    for (int i = g; i < tiles; i += G) s0 += gap[((size_t)b * tiles + i) * C + c];
#pragma unroll 4
    for (int x = g; x < W; x += G) {
        s1 += tb[(size_t)x * C + c];
        s2 += tb[((size_t)(H - 1) * W + x) * C + c];
    }
#pragma unroll 4
    for (int y = g; y < H; y += G) {
        s3 += tb[((size_t)y * W) * C + c];
        s4 += tb[((size_t)y * W + W - 1) * C + c];
    }
    part[t] = s0; part[GP_T + t] = s1; part[2 * GP_T + t] = s2; part[3 * GP_T + t] = s3; part[4 * GP_T + t] = s4;
    __syncthreads();
    if (t < C) {
        float T = 0.f, R0 = 0.f, RL = 0.f, C0 = 0.f, CL = 0.f;
        for (int j = 0; j < G; ++j) {
            T += part[j * C + t]; R0 += part[GP_T + j * C + t]; RL += part[2 * GP_T + j * C + t]; C0 += part[3 * GP_T + j * C + t];
            CL += part[4 * GP_T + j * C + t];
        }
        const float c00 = tb[t], c0L = tb[(size_t)(W - 1) * C + t], cL0 = tb[((size_t)(H - 1) * W) * C + t], cLL = tb[((size_t)(H - 1) * W + W - 1) * C + t];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const float rex = kh == 0 ? RL : (kh == 2 ? R0 : 0.f);
                const float cex = kw == 0 ? CL : (kw == 2 ? C0 : 0.f);
                float corner = 0.f;
                if (kh == 0 && kw == 0) corner = cLL;
                if (kh == 0 && kw == 2) corner = cL0;
                if (kh == 2 && kw == 0) corner = c0L;
                if (kh == 2 && kw == 2) corner = c00;
                S[(kh * 3 + kw) * C + t] = T - rex - cex + corner;
            }
    }
    __syncthreads();
    {   // z[co] = sum over (tap, ci) of W[tap][ci/4][co][4] * S[tap][ci]; the 9*C/4 quads are dealt to the G thread groups
        const f4* w4 = reinterpret_cast<const f4*>(w2img);
        const int nq = 9 * (C >> 2);
        float z = 0.f;
#pragma unroll 4
        for (int q = g; q < nq; q += G) {
            const int tap = q / (C >> 2), cq = q - tap * (C >> 2);
            const f4 wv = w4[(size_t)q * C + c];
            const float* sp = S + tap * C + cq * 4;
            z += (wv[0] * sp[0] + wv[1] * sp[1]) + (wv[2] * sp[2] + wv[3] * sp[3]);
        }
        zp[g * C + c] = z;
    }
    __syncthreads();
    if (t < C) {
        float z = 0.f;
        for (int j = 0; j < G; ++j) z += zp[j * C + t];
        m[t] = z / (float)(H * W) * scale2[t] + shift2[t];
    }
    __syncthreads();
    {   // hidden layer: one wave per unit, lanes stride the C inputs, fixed-order wave reduction (R threads each walking a row of W1 was a
        // 2.5 us serial chain at C = 128: stamps in profiles/r06_gate_pre_stamps.txt)
        const int wv = t >> 6, lane = t & 63;
        for (int j = wv; j < R; j += GP_T / 64) {
            float s = 0.f;
            for (int cc = lane; cc < C; cc += 64) s += w1[j * C + cc] * m[cc];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) hbuf[j] = fmaxf(s + b1[j], 0.f);
        }
    }
    __syncthreads();
    if (t < C) {
        float s = bf2[t];
        for (int j = 0; j < R; ++j) s += wf2[t * R + j] * hbuf[j];
        const float gt = 1.f / (1.f + expf(-s));
        gate[(size_t)b * C + t] = gt;
        if (sc_vec) {
            // a block with a downsample shortcut (conv3x3_bf16_kernel, SCC): conv2 scales its shortcut product D by f = sd / q before the 3x3 taps and its
            // epilogue computes relu(acc * q + h), q = gate * s2, h = h2 * gate + hd.  |q| is kept >= 1e-30 (sign kept; q = 0 counts as positive) so that
            // f stays finite: D * sd / 1e-30 is inside fp32 for any |D * sd| < 1e8.  The SAME clamped q multiplies the accumulator again in the epilogue,
            // so the shortcut comes back as D * sd exactly (to rounding), and what the clamp distorts is the conv2 term alone, by less than
            // 1e-30 * |conv2|: the output error stays at rounding level, also for bn2.weight == 0 or a gate that underflows.
            const size_t BC = (size_t)gridDim.x * C;
            float q = gt * scale2[t];
            if (!(fabsf(q) >= 1e-30f)) q = copysignf(1e-30f, q);
            sc_vec[(size_t)b * C + t] = ds_scale[t] / q;
            sc_vec[BC + (size_t)b * C + t] = q;
            sc_vec[2 * BC + (size_t)b * C + t] = shift2[t] * gt + ds_shift[t];
        }
    }
}

// ---- SE tail: out = relu(y*gate + residual) ----------------------------------------------------------
__global__ __launch_bounds__(256) void se_tail_identity_kernel(const f4* __restrict__ y, const float* __restrict__ gate,
                                                               const f4* __restrict__ res, f4* __restrict__ out,
                                                               size_t n4, int hw_cq, int cq_n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const int cq = (int)(i % cq_n);
        const size_t b = i / hw_cq;
        const f4 g = *reinterpret_cast<const f4*>(gate + b * cq_n * 4 + cq * 4);
        f4 v = y[i] * g + res[i];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        out[i] = v;
    }
}

// residual = BN(conv1x1 stride s (x_in)); weights [CIN][COUT] staged in LDS; one thread = 1 pixel x 4 couts
template <int CIN, int COUT>
__global__ __launch_bounds__(256) void se_tail_downsample_kernel(const float* __restrict__ y, const float* __restrict__ gate,
                                                                 const float* __restrict__ xin, const float* __restrict__ dsw,
                                                                 const float* __restrict__ dss, const float* __restrict__ dsh,
                                                                 float* __restrict__ out, int B, int Ho, int Wo, int Hin, int Win, int S) {
    extern __shared__ __attribute__((aligned(16))) f4 wl[];         // CIN * COUT / 4 (128 KB at 128 -> 256)
    for (int i = threadIdx.x; i < CIN * COUT / 4; i += 256) wl[i] = reinterpret_cast<const f4*>(dsw)[i];
    __syncthreads();
    constexpr int CQ = COUT / 4;
    // rows of the output map are dealt to the workgroups; inside a row the index splits by shifts (CQ is a power of two): no per-element
    // 64-bit division (three per output quad in the first version)
    for (int row = blockIdx.x; row < B * Ho; row += gridDim.x) {
      const int b = row / Ho, oy = row - b * Ho;
      for (int t = threadIdx.x; t < Wo * CQ; t += 256) {
        const int cq = t % CQ, ox = t / CQ;
        const size_t p = (size_t)row * Wo + ox;
        const float* xp = xin + (((size_t)b * Hin + (size_t)oy * S) * Win + (size_t)ox * S) * CIN;
        f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int ci = 0; ci < CIN; ci += 4) {
            const f4 xv = *reinterpret_cast<const f4*>(xp + ci);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += wl[(ci + j) * CQ + cq] * xv[j];
        }
        const f4 res = acc * *reinterpret_cast<const f4*>(dss + cq * 4) + *reinterpret_cast<const f4*>(dsh + cq * 4);
        const f4 g = *reinterpret_cast<const f4*>(gate + (size_t)b * COUT + cq * 4);
        f4 v = *reinterpret_cast<const f4*>(y + p * COUT + cq * 4) * g + res;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        *reinterpret_cast<f4*>(out + p * COUT + cq * 4) = v;
      }
    }
}

// ---- launch functions ---------------------------------------------------------------------------------------------------------------
// A launch with dynamic LDS: opt the kernel in past 64 KB (once per kernel and device), launch 256 threads per workgroup, check.
template <typename K, typename... Args>
int launch_dyn(K kernel, dim3 grid, size_t lds_bytes, const char* what, hipStream_t st, const Args&... args) {
    if (int rc = eg_ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), lds_bytes, what)) return rc;
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds_bytes, st, args...);
    return eg_check_launch(what);
}

// The split-bf16 images of a packed 3x3 weight (eg_conv3x3_packed_floats): [fp32 image: 9 * cin * coutp floats][hi: 9 * cin / 8 * coutp octets][lo: the same].
// The only place that knows the arena layout behind the fp32 image.
struct PackedImages { const bf8* whi; const bf8* wlo; };
PackedImages packed_images(const float* w, int cin, int coutp) {
    const bf8* whi = reinterpret_cast<const bf8*>(w + (size_t)9 * cin * coutp);
    return {whi, whi + (size_t)9 * (cin / 8) * coutp};
}

// ---- routes ---------------------------------------------------------------------------------------------------------------------------
// One entry per supported (input channels, stride, output channels).  `rows` is the tile height that sizes the grid AND the layout of the pooling partials
// (eg_conv3x3_gap_tiles: callers size their buffers from it), wm x wn the wave grid (pixels x channels) of the tiled kernels, `split` the largest channel
// split.  The launch functions below take their template arguments from here, so a launch and its buffers cannot disagree.
struct ConvRoute {
    int cin, stride, cout_lo, cout_hi, rows, wm, wn, split = 1;
    constexpr int nt() const { return (cout_hi + 15) / 16; }        // 16-channel tiles of the padded output channels (the row length of the packed images)
};
enum { R_32, R_32_NARROW, R_32_64, R_64, R_64_128, R_64_128_S1, R_128, R_128_64, R_128_48, R_128_256, R_256, NROUTES };
constexpr ConvRoute ROUTES[NROUTES] = {
    {.cin = 32, .stride = 1, .cout_lo = 32, .cout_hi = 32, .rows = 4, .wm = 4, .wn = 1},        // HBM-bound first stage: smaller LDS footprint, more workgroups in flight
    {.cin = 32, .stride = 1, .cout_lo = 17, .cout_hi = 31, .rows = 8, .wm = 4, .wn = 1},
    {.cin = 32, .stride = 2, .cout_lo = 49, .cout_hi = 64, .rows = 2, .wm = 2, .wn = 2},        // stage entry
    {.cin = 64, .stride = 1, .cout_lo = 49, .cout_hi = 64, .rows = 8, .wm = 4, .wn = 1, .split = 2},
    {.cin = 64, .stride = 2, .cout_lo = 113, .cout_hi = 128, .rows = 2, .wm = 2, .wn = 2},      // stage entry
    {.cin = 64, .stride = 1, .cout_lo = 128, .cout_hi = 128, .rows = 4, .wm = 2, .wn = 2},      // training: input gradient of final_conv1 (dy padded to 64 channels)
    {.cin = 128, .stride = 1, .cout_lo = 65, .cout_hi = 128, .rows = 4, .wm = 2, .wn = 2, .split = 4},      // body; final_conv1 with 65 .. 128 frames on zero-padded weights
    {.cin = 128, .stride = 1, .cout_lo = 49, .cout_hi = 64, .rows = 4, .wm = 4, .wn = 1},       // final_conv1: 128 -> frames (60 -> 64)
    {.cin = 128, .stride = 1, .cout_lo = 1, .cout_hi = 48, .rows = 4, .wm = 4, .wn = 1},        // final_conv1 (34 -> 48)
    // 256-channel stage of the audio emotion classifier (model/audio_emotion_classifer.py:20-22): 2-row tiles, waves split the channels
    {.cin = 128, .stride = 2, .cout_lo = 241, .cout_hi = 256, .rows = 2, .wm = 1, .wn = 4},
    {.cin = 256, .stride = 1, .cout_lo = 256, .cout_hi = 256, .rows = 2, .wm = 1, .wn = 4},
};
constexpr int route_index(int cin, int cout, int stride) {      // NROUTES: no kernel serves the shape
    int i = 0;
    while (i < NROUTES && !(ROUTES[i].cin == cin && ROUTES[i].stride == stride && cout >= ROUTES[i].cout_lo && cout <= ROUTES[i].cout_hi)) ++i;
    return i;
}
// eg_conv3x3_gap_tiles answers for every shape (callers size buffers first): a route's `rows`, else this rule, which on the routes gives `rows` too (checked below)
constexpr int unserved_tile_rows(int cin, int cout, int stride) {
    if (stride == 2 || cout >= 256) return 2;
    if (cin == 32 && cout == 32) return 4;
    return (cout >= 128 || cin >= 128) ? 4 : 8;
}
constexpr int conv_tile_rows(int cin, int cout, int stride) {
    const int i = route_index(cin, cout, stride);
    return i < NROUTES ? ROUTES[i].rows : unserved_tile_rows(cin, cout, stride);
}
constexpr bool routes_keep_the_tile_rows() {
    for (const ConvRoute& r : ROUTES)
        for (int cout = r.cout_lo; cout <= r.cout_hi; ++cout)
            if (r.rows != unserved_tile_rows(r.cin, cout, r.stride)) return false;
    return true;
}
static_assert(routes_keep_the_tile_rows(), "a route's tile height differs from what eg_conv3x3_gap_tiles has always answered for its shapes");
static_assert(ROUTES[R_32].rows == C32_ROWS, "the persistent walk writes the route's partial layout");

// Route I's tiled kernel, one workgroup per rows x 32 tile and all output channels (conv3x3_f32_kernel, or conv3x3_bf16_kernel on the route's wave grid).
// SCC > 0: conv2 of a stage-entry block, which contracts SCC 32-channel chunks of the block input through the 1x1 downsample shortcut itself.
template <int I, int SCC = 0>
int launch_conv(const ConvArgs& a, int batch, int precision, hipStream_t st) {
    constexpr ConvRoute R = ROUTES[I];
    const dim3 grid(a.tiles, batch);
    if (precision == EG_PREC_F32) {
        if constexpr (SCC > 0) {
            eg_set_error("conv3x3: the fused downsample shortcut exists in the split-bf16 modes only");
            return EG_ERR_UNSUPPORTED;
        }
        hipLaunchKernelGGL((conv3x3_f32_kernel<R.cin, R.nt(), R.stride, R.rows>), grid, dim3(256), 0, st, a);
        return eg_check_launch("conv3x3");
    }
    const PackedImages p = packed_images(a.w, R.cin, R.nt() * 16);
    constexpr int PL = ConvBf16Geom<R.stride, R.rows, false>::PL;
    if (precision == EG_PREC_BF16X3)
        return launch_dyn(conv3x3_bf16_kernel<R.cin, R.nt(), R.stride, R.rows, R.wm, R.wn, 3, false, false, SCC>, grid, RingLds<PL, R.nt() * 16, 3>::BYTES, "conv3x3", st, a, p.whi, p.wlo);
    return launch_dyn(conv3x3_bf16_kernel<R.cin, R.nt(), R.stride, R.rows, R.wm, R.wn, 1, false, false, SCC>, grid, RingLds<PL, R.nt() * 16, 1>::BYTES, "conv3x3", st, a, p.whi, p.wlo);
}
// Channel-split launch of a stride-1 C -> C body convolution (bf16x3): 1 / SPLIT of the output channels per workgroup, grid.z = SPLIT; bitwise the unsplit kernel
template <int I, int SPLIT, int SCC = 0>
int launch_conv_split(ConvArgs a, int batch, hipStream_t st) {
    constexpr ConvRoute R = ROUTES[I];
    constexpr int NTS = R.nt() / SPLIT;
    const PackedImages p = packed_images(a.w, R.cin, a.cout);
    a.wrow = a.cout;
    return launch_dyn(conv3x3_bf16_kernel<R.cin, NTS, 1, R.rows, R.wm, R.wn, 3, true, false, SCC>, dim3(a.tiles, batch, SPLIT),
                      RingLds<ConvBf16Geom<1, R.rows, false>::PL, NTS * 16, 3>::BYTES, "conv3x3 (channel split)", st, a, p.whi, p.wlo);
}
// Input gradient of a stride-2 convolution (conv3x3_bf16_kernel, DG2): KCH = the convolution's output channels (the contraction), NTN * 16 = its input
// channels; grid over TH x 32 tiles of the dy grid.
template <int KCH, int NTN, int TH, int WM, int WN>
int launch_dgrad_s2(const ConvArgs& a, int batch, hipStream_t st) {
    const PackedImages p = packed_images(a.w, KCH, NTN * 16);        // the flipped image: KCH "input" channels -> NTN * 16 "output" channels
    return launch_dyn(conv3x3_bf16_kernel<KCH, NTN, 1, TH, WM, WN, 3, false, true>, dim3(eg_cdiv(a.W, 32) * eg_cdiv(a.H, TH), batch),
                      RingLds<ConvBf16Geom<1, TH, true>::PL, NTN * 16, 3>::BYTES, "conv3x3 (stride-2 input gradient)", st, a, p.whi, p.wlo);
}
// how many ways to split the channels of a C -> C body convolution with `wgs` pixel-tile workgroups: keep the launch near one workgroup per CU
int conv_channel_split(int wgs, int max_split) {
    const char* e = getenv("EG_CONV_SPLIT");            // A/B switch, read per call: 1 = never, 2, 4 (a captured graph keeps what it was captured with)
    const int forced = (e && e[0]) ? atoi(e) : -1;
    if (forced >= 0) return (forced == 2 || forced == 4) && forced <= max_split ? forced : 1;
    // measured (tools/conv_b1_probe.py, us per launch, unsplit / 2 / 4): 128 ch. 64 tiles 26.9 / 18.9 / 15.3, 128 tiles 28.6 / 20.7 / 20.8, 256 tiles
    // 31.1 / 30.7 / 37.0; 64 ch. 128 tiles 18.4 / 13.9, 256 tiles 20.1 / 19.6, 512 tiles 29.7 / 37.6 -- split while the launch stays within two workgroups per CU
    int split = 1;
    while (split < max_split && wgs * split * 2 <= 512) split *= 2;
    return split;
}
// the channel split a C -> C body convolution takes (1: none; the split kernels exist for bf16x3 and NHWC output)
int body_channel_split(int batch, int tiles, int cin, int cout, int stride, int precision, int nchw_out) {
    const int i = route_index(cin, cout, stride);
    if (i == NROUTES || cout != cin || precision != EG_PREC_BF16X3 || nchw_out) return 1;
    return conv_channel_split(tiles * batch, ROUTES[i].split);
}

// A stage-entry route (32 -> 64, 64 -> 128, stride 2) on parity planes (conv3x3_s2_planes_kernel): TH x 32 output tiles, a wave per 2 x 32 output block of
// its channel range (wave grid TH / 2 x 8 / TH).
template <int I, int TH>
int launch_conv_s2_planes(const ConvArgs& a, int batch, int precision, hipStream_t st) {
    constexpr int CIN = ROUTES[I].cin, NTT = ROUTES[I].nt(), WM = TH / 2, WN = 4 / WM, PL = ConvGeomS2P<TH>::PL;
    static_assert(ROUTES[I].rows == 2, "the plane walk writes the partials of 2 x 32 blocks (conv_s2_form)");
    const PackedImages p = packed_images(a.w, CIN, NTT * 16);
    const dim3 grid(a.tiles_x * eg_cdiv(a.Ho, TH), batch);
    auto go = [&](auto kern, size_t lds_bytes) { return launch_dyn(kern, grid, lds_bytes, "conv3x3 (stride 2, planes)", st, a, p.whi, p.wlo); };
    // the training path's input affine has instantiations of its own, so that the inference kernels carry none of it
    if (precision == EG_PREC_BF16X3)
        return a.in_scale ? go(conv3x3_s2_planes_kernel<CIN, NTT, TH, WM, WN, 3, true>, RingLds<PL, NTT * 16, 3>::BYTES)
                          : go(conv3x3_s2_planes_kernel<CIN, NTT, TH, WM, WN, 3, false>, RingLds<PL, NTT * 16, 3>::BYTES);
    return a.in_scale ? go(conv3x3_s2_planes_kernel<CIN, NTT, TH, WM, WN, 1, true>, RingLds<PL, NTT * 16, 1>::BYTES)
                      : go(conv3x3_s2_planes_kernel<CIN, NTT, TH, WM, WN, 1, false>, RingLds<PL, NTT * 16, 1>::BYTES);
}
// Which form a stage-entry convolution takes: 0 = interleaved halo (conv3x3_bf16_kernel, S = 2, the route's 2-row tiles), else the tile height of the plane walk.
// The larger tiles belong to that form alone: its pooling partials keep the route's 2-row layout, so eg_conv3x3_gap_tiles is the same for both forms.
// EG_CONV_S2 is an A/B switch read per call (a captured graph keeps what it was captured with): "interleaved"; "planes" (the plane walk at every
// size); "planes4" / "planes8" (the same with the 32 -> 64 entry's tile height forced; the 64 -> 128 entry has 4-row tiles only); unset = by size.
// Measured alone (TED shapes, bf16x3, us per launch at 1 / 8 / 16 / 32 / 64 clips; profiles/r13_stride2_planes_ab.txt):
//   32 -> 64:  interleaved 7.1 / 11.5 / 19.7 / 38.1 / 73.3   4-row planes 9.8 / 12.4 / 14.9 / 31.5 / 55.0   8-row planes 15.1 / 17.0 / 18.9 / 25.2 / 55.4
//   64 -> 128: interleaved 13.2 / 14.9 / 16.4 / 29.5 / 59.1  4-row planes 19.1 / 21.1 / 21.8 / 23.4 / 34.9
// A plane-walk workgroup lives longer than an interleaved one (four plane swaps per chunk), which pays once the launch fills the chip: the
// interleaved form stays below 256 workgroups of the plane walk (8-row tiles counted for 32 -> 64), 8-row tiles start at 512.
int conv_s2_form(int cin, int batch, int ho, int wo) {
    const char* e = getenv("EG_CONV_S2");
    if (e && !strcmp(e, "interleaved")) return 0;
    const bool forced = e && !strncmp(e, "planes", 6);
    const int wgs = eg_cdiv(wo, 32) * eg_cdiv(ho, cin == 64 ? 4 : 8) * batch;
    if (!forced && wgs < 256) return 0;
    if (cin == 64) return 4;
    if (e && !strcmp(e, "planes4")) return 4;
    if (e && !strcmp(e, "planes8")) return 8;
    return wgs >= 512 ? 8 : 4;
}

bool conv32_persistent_enabled() {
    static const bool on = [] { const char* e = getenv("EG_CONV32_PERSISTENT"); return !(e && e[0] == '0'); }();
    return on;
}
int launch_conv32_persistent(const ConvArgs& a, int batch, int precision, hipStream_t st) {
    const PackedImages p = packed_images(a.w, 32, 32);
    const int total = a.tiles * batch;
    // 512 = 2 workgroups per CU, each walking total / 512 tiles (more, shorter-lived workgroups were measured slower alone and under four lanes:
    // profiles/r05_conv32_experiments.txt).
    int grid = total < 512 ? total : 512;
    grid = eg_cdiv(total, eg_cdiv(total, grid));
    if (grid >= 8) grid = (int)eg_round_up(grid, 8);             // XCD remap needs a multiple of 8 (surplus workgroups exit at once)
    const char* what = "conv3x3 (32 -> 32, persistent)";
    if (precision == EG_PREC_BF16X3) return launch_dyn(conv3x3_c32_persistent_kernel<3>, dim3(grid), C32Lds<3>::BYTES, what, st, a, p.whi, p.wlo, total);
    return launch_dyn(conv3x3_c32_persistent_kernel<1>, dim3(grid), C32Lds<1>::BYTES, what, st, a, p.whi, p.wlo, total);
}

// the downsample shortcut conv2 of a stage-entry block contracts itself (conv3x3_bf16_kernel, SCC): block input x [B][h][w][cin], the packed 1x1 images
// (EG_PACK_CONV1X1_BF16) and the per-clip vectors [f | q | h] of se_gate_pre_kernel
struct ShortcutArgs { const float* x; const float* wimg; const float* vec; int h, w, cin, stride; };
// what an entry point asks of conv3x3_dispatch: of `a` it fills the operands, H, W, cout, relu and nchw; the dispatch derives the rest
struct ConvRequest {
    ConvArgs a;
    int batch, cin, stride, precision;
    void* stream;
    const ShortcutArgs* sc = nullptr;
};

int conv3x3_dispatch(ConvRequest q) {
    ConvArgs& a = q.a;
    const int batch = q.batch, h = a.H, wdt = a.W, cin = q.cin, cout = a.cout, stride = q.stride, precision = q.precision;
    const ShortcutArgs* sc = q.sc;
    EG_REQUIRE(a.x && a.w && a.y && batch > 0 && h > 0 && wdt > 0, EG_ERR_BAD_ARG, "eg_conv3x3: null pointer or empty shape");
    EG_REQUIRE(!a.res_bits || (a.res && !a.gate && ((size_t)batch * h * wdt * cout) % 32 == 0), EG_ERR_BAD_ARG,
               "eg_conv3x3_res_masked: the bit mask needs a residual, no gate and a map of a multiple of 32 elements");
    EG_REQUIRE((a.in_scale == nullptr) == (a.in_shift == nullptr) && (!a.in_scale || (precision != EG_PREC_F32 && cin % 32 == 0 && eg_aligned16(a.in_scale) &&
               eg_aligned16(a.in_shift))), EG_ERR_BAD_ARG, "eg_conv3x3: the input affine needs both vectors, a split-bf16 mode and cin %% 32 == 0");
    // gate + residual: relu(v * gate + residual) (the fused SE tail); residual alone: v + residual, no ReLU (the training path's fused fan-in add:
    // an input gradient that lands on a tensor with a second consumer, train/functional.py conv3x3(passthrough=True))
    EG_REQUIRE(!a.gate || a.res, EG_ERR_BAD_ARG, "eg_conv3x3_se: a gate needs a residual");
    EG_REQUIRE(!a.res || (!a.nchw && stride == 1 && cout % 4 == 0 && (!a.gate || eg_aligned16(a.gate)) && eg_aligned16(a.res) && a.res != a.y),
               EG_ERR_BAD_ARG, "eg_conv3x3_se: the fused residual needs NHWC output, stride 1, cout %% 4 == 0 and a residual buffer distinct from y");
    EG_REQUIRE(eg_aligned16(a.x) && eg_aligned16(a.w) && eg_aligned16(a.y), EG_ERR_ALIGN, "eg_conv3x3: pointers must be 16-byte aligned");
    EG_REQUIRE(stride == 1 || stride == 2, EG_ERR_UNSUPPORTED, "eg_conv3x3: stride %d", stride);
    EG_REQUIRE(precision >= 0 && precision <= 2, EG_ERR_BAD_ARG, "eg_conv3x3: precision %d", precision);
    EG_REQUIRE(a.nchw || (cout % 4 == 0), EG_ERR_UNSUPPORTED, "eg_conv3x3: NHWC output needs cout %% 4 == 0");
    a.relu2 = a.gate ? 1 : 0;
    a.Ho = (h + 2 - 3) / stride + 1; a.Wo = (wdt + 2 - 3) / stride + 1;
    a.tiles_x = eg_cdiv(a.Wo, 32);
    a.tiles = a.tiles_x * eg_cdiv(a.Ho, conv_tile_rows(cin, cout, stride));
    hipStream_t st = (hipStream_t)q.stream;
    EgProfScope prof((int64_t)cin * 1000000 + (int64_t)cout * 1000 + stride * 100 + 1,
                     2.0 * 9 * cin * cout * (double)a.Ho * a.Wo * batch, st);
    if (sc) {
        EG_REQUIRE(precision != EG_PREC_F32 && stride == 1 && !a.nchw && cout == cin && (cin == 64 || cin == 128) && sc->cin * 2 == cin, EG_ERR_UNSUPPORTED,
                   "conv3x3: the fused downsample shortcut serves 32 -> 64 and 64 -> 128 block entries in the split-bf16 modes (cin=%d cout=%d shortcut cin=%d)",
                   cin, cout, sc->cin);
        EG_REQUIRE(sc->x && sc->wimg && sc->vec && !a.gate && !a.res && !a.bias && !a.relu && !a.gap2 && !a.in_scale && sc->stride >= 1 &&
                   (sc->h - 1) / sc->stride + 1 == h && (sc->w - 1) / sc->stride + 1 == wdt && eg_aligned16(sc->x) && eg_aligned16(sc->wimg) &&
                   eg_aligned16(sc->vec), EG_ERR_BAD_ARG, "conv3x3: fused downsample shortcut: null / misaligned operand or a block input that does not map onto the output");
        a.sc_x = sc->x; a.sc_vec = sc->vec; a.sc_H = sc->h; a.sc_W = sc->w; a.sc_S = sc->stride; a.sc_B = batch;
        a.sc_whi = reinterpret_cast<const bf8*>(sc->wimg);       // the packed 1x1 images: [ci/8][co][8], hi then lo
        a.sc_wlo = a.sc_whi + (size_t)(sc->cin / 8) * cout;
        a.scale = a.shift = nullptr;             // the epilogue's scale and shift are the per-clip q and h
        a.relu2 = 1;
    }
    // forms that replace the route's tiled kernel, bit for bit: a small body launch's channel split; a stage entry's plane walk (not fp32, NCHW, padded channels)
    const int split = body_channel_split(batch, a.tiles, cin, cout, stride, precision, a.nchw);
    const int s2p = (stride == 2 && cout % 16 == 0 && precision != EG_PREC_F32 && !a.nchw && (!a.gap || eg_aligned16(a.gap)) && (!a.gap2 || eg_aligned16(a.gap2)))
                        ? conv_s2_form(cin, batch, a.Ho, a.Wo) : 0;
    switch (route_index(cin, cout, stride)) {
    case R_32: {
        // the retired 8-row tiles (tools/experiments/README.md) are refused, read per call: a stale A/B script must not measure the default under the old name
        const char* th = getenv("EG_CONV32_TH");
        EG_REQUIRE(!(th && th[0] && strcmp(th, "4") != 0), EG_ERR_BAD_ARG, "eg_conv3x3: EG_CONV32_TH=%s: the 8-row tiles of the 32 -> 32 kernel are retired "
                   "(tools/experiments/README.md); unset it or set 4", th);
        if (precision != EG_PREC_F32 && !a.nchw && conv32_persistent_enabled()) return launch_conv32_persistent(a, batch, precision, st);
        return launch_conv<R_32>(a, batch, precision, st);
    }
    case R_32_64:
        if (s2p == 8) return launch_conv_s2_planes<R_32_64, 8>(a, batch, precision, st);
        if (s2p == 4) return launch_conv_s2_planes<R_32_64, 4>(a, batch, precision, st);
        return launch_conv<R_32_64>(a, batch, precision, st);
    case R_64_128:
        if (s2p == 4) return launch_conv_s2_planes<R_64_128, 4>(a, batch, precision, st);
        return launch_conv<R_64_128>(a, batch, precision, st);
    case R_64:
        if (sc) return split == 2 ? launch_conv_split<R_64, 2, 1>(a, batch, st) : launch_conv<R_64, 1>(a, batch, precision, st);
        return split == 2 ? launch_conv_split<R_64, 2>(a, batch, st) : launch_conv<R_64>(a, batch, precision, st);
    case R_128:
        if (sc && split == 4) return launch_conv_split<R_128, 4, 2>(a, batch, st);
        if (sc) return split == 2 ? launch_conv_split<R_128, 2, 2>(a, batch, st) : launch_conv<R_128, 2>(a, batch, precision, st);
        if (split == 4) return launch_conv_split<R_128, 4>(a, batch, st);
        return split == 2 ? launch_conv_split<R_128, 2>(a, batch, st) : launch_conv<R_128>(a, batch, precision, st);
    case R_32_NARROW: return launch_conv<R_32_NARROW>(a, batch, precision, st);
    case R_64_128_S1: return launch_conv<R_64_128_S1>(a, batch, precision, st);
    case R_128_64: return launch_conv<R_128_64>(a, batch, precision, st);
    case R_128_48: return launch_conv<R_128_48>(a, batch, precision, st);
    case R_128_256: return launch_conv<R_128_256>(a, batch, precision, st);
    case R_256: return launch_conv<R_256>(a, batch, precision, st);
    }
    eg_set_error("eg_conv3x3: unsupported channels cin=%d cout=%d stride=%d", cin, cout, stride);
    return EG_ERR_UNSUPPORTED;
}

}  // namespace

extern "C" int32_t eg_conv3x3_gap_tiles(int32_t h, int32_t wdt, int32_t cin, int32_t cout, int32_t stride) {
    const int ho = (h + 2 - 3) / stride + 1, wo = (wdt + 2 - 3) / stride + 1;
    return eg_cdiv(ho, conv_tile_rows(cin, cout, stride)) * eg_cdiv(wo, 32);
}

// The row length of the packed images (and of bias / scale / shift) the route's kernels read: fixed by the route, not by cout.  0: no route serves the shape.
extern "C" int32_t eg_conv3x3_cout_pad(int32_t cin, int32_t cout, int32_t stride) {
    const int i = route_index(cin, cout, stride);
    return i < NROUTES ? ROUTES[i].nt() * 16 : 0;
}

// The channel split eg_conv3x3 (and every entry point that shares its dispatch: _se, _sq, _sq_in_affine, _res_masked) takes for this launch.
extern "C" int32_t eg_conv3x3_channel_split(int32_t batch, int32_t h, int32_t wdt, int32_t cin, int32_t cout, int32_t stride, int32_t precision) {
    return body_channel_split(batch, eg_conv3x3_gap_tiles(h, wdt, cin, cout, stride), cin, cout, stride, precision, 0);
}

// Packed weight size in floats for one 3x3 conv: fp32 image + (hi, lo) bf16 images.
extern "C" int64_t eg_conv3x3_packed_floats(int32_t cin, int32_t cout_pad) {
    return (int64_t)9 * cin * cout_pad * 2;     // 9*cin*coutp fp32 + 2 * 9*cin*coutp bf16 (= same bytes again)
}

extern "C" int eg_conv3x3(const float* x, const float* w, const float* bias, const float* scale, const float* shift,
                          float* y, float* gap_partial, int32_t batch, int32_t h, int32_t wdt, int32_t cin, int32_t cout,
                          int32_t stride, int32_t relu, int32_t nchw_out, int32_t precision, void* stream) {
    return eg_conv3x3_se(x, w, bias, scale, shift, nullptr, nullptr, y, gap_partial, batch, h, wdt, cin, cout, stride, relu, nchw_out, precision, stream);
}

extern "C" int eg_conv3x3_se(const float* x, const float* w, const float* bias, const float* scale, const float* shift, const float* gate,
                             const float* residual, float* y, float* gap_partial, int32_t batch, int32_t h, int32_t wdt, int32_t cin,
                             int32_t cout, int32_t stride, int32_t relu, int32_t nchw_out, int32_t precision, void* stream) {
    return conv3x3_dispatch({.a = {.x = x, .w = w, .bias = bias, .scale = scale, .shift = shift, .y = y, .gap = gap_partial, .H = h, .W = wdt, .cout = cout,
                                   .relu = relu, .nchw = nchw_out, .gate = gate, .res = residual},
                             .batch = batch, .cin = cin, .stride = stride, .precision = precision, .stream = stream});
}
// y = conv(x) + (bit ? residual : 0): the input gradient of an SE block's first convolution with the identity shortcut's gradient
// dout * (out > 0) (ResNetBlocks.py:33-36) added in the epilogue straight from dout and the tail's ReLU bits (csrc/train.hip: se_tail_fwd_kernel writes one bit
// per element, bit e & 31 of word e >> 5) -- the masked map is never stored.  Stride 1, NHWC, cout % 4 == 0; x is the upstream gradient, w the flipped image.
extern "C" int eg_conv3x3_res_masked(const float* x, const float* w, const float* residual, const uint32_t* res_bits, float* y, int32_t batch, int32_t h,
                                     int32_t wdt, int32_t cin, int32_t cout, int32_t precision, void* stream) {
    EG_REQUIRE(residual && res_bits, EG_ERR_BAD_ARG, "eg_conv3x3_res_masked: the residual and its bit mask are required");
    return conv3x3_dispatch({.a = {.x = x, .w = w, .y = y, .H = h, .W = wdt, .cout = cout, .res = residual, .res_bits = res_bits},
                             .batch = batch, .cin = cin, .stride = 1, .precision = precision, .stream = stream});
}
// Training forward: y = [relu](conv(x) + bias), plus the per-(clip, tile) channel sums of y AND of y*y (both [batch][tiles][cout]): train-mode
// BatchNorm takes its mean and variance from them (csrc/train.hip: eg_bn_train_forward_sq) without reading y again.  Split-bf16 modes only.
extern "C" int eg_conv3x3_sq(const float* x, const float* w, const float* bias, float* y, float* gap_partial, float* gap_sq_partial, int32_t batch, int32_t h,
                             int32_t wdt, int32_t cin, int32_t cout, int32_t stride, int32_t relu, int32_t precision, void* stream) {
    EG_REQUIRE(gap_partial && gap_sq_partial, EG_ERR_BAD_ARG, "eg_conv3x3_sq: both partial buffers are required");
    EG_REQUIRE(precision != EG_PREC_F32, EG_ERR_UNSUPPORTED, "eg_conv3x3_sq: split-bf16 modes only (the fp32 kernel emits sums only)");
    return conv3x3_dispatch({.a = {.x = x, .w = w, .bias = bias, .y = y, .gap = gap_partial, .gap2 = gap_sq_partial, .H = h, .W = wdt, .cout = cout, .relu = relu},
                             .batch = batch, .cin = cin, .stride = stride, .precision = precision, .stream = stream});
}
// eg_conv3x3_sq on x' = x * in_scale[ci] + in_shift[ci] (per INPUT channel, in-image pixels; the zero padding stays zero): the train-mode BatchNorm in
// front of the convolution folded into its operand staging, so that the normalised map is never written (ResNetBlocks.py:26-27: bn1 -> conv2).
extern "C" int eg_conv3x3_sq_in_affine(const float* x, const float* in_scale, const float* in_shift, const float* w, const float* bias, float* y,
                                       float* gap_partial, float* gap_sq_partial, int32_t batch, int32_t h, int32_t wdt, int32_t cin, int32_t cout,
                                       int32_t stride, int32_t relu, int32_t precision, void* stream) {
    EG_REQUIRE(in_scale && in_shift, EG_ERR_BAD_ARG, "eg_conv3x3_sq_in_affine: both affine vectors are required");
    EG_REQUIRE(!gap_partial == !gap_sq_partial, EG_ERR_BAD_ARG, "eg_conv3x3_sq_in_affine: both partial buffers or none");
    return conv3x3_dispatch({.a = {.x = x, .w = w, .bias = bias, .y = y, .gap = gap_partial, .gap2 = gap_sq_partial, .H = h, .W = wdt, .cout = cout, .relu = relu,
                                   .in_scale = in_scale, .in_shift = in_shift},
                             .batch = batch, .cin = cin, .stride = stride, .precision = precision, .stream = stream});
}

// dx = F.conv2d's input gradient of nn.Conv2d(cin -> cout, k = 3, pad = 1, stride = 2) (the `_make_layer` entry convolutions, ResNetSE34V2.py:40-55):
// dy [batch][ho][wo][cout], w_flip = the packed images of the rotated, transposed filter (cout -> cin: the image the stride-1 input gradients use),
// dx [batch][h][w][cin] with ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1.  res_q (optional): a gradient [batch][ho][wo][cin] that belongs to the
// pixels (2i, 2j) of dx -- the stride-2 1x1 shortcut's input gradient (:43-47) -- added in the epilogue instead of scattered into a zero map.
// Split-bf16 (EG_PREC_BF16X3) only; (cin, cout) in {(32, 64), (64, 128), (128, 256)}.  Every element of dx is written.
extern "C" int eg_conv3x3_dgrad_s2(const float* dy, const float* w_flip, const float* res_q, float* dx, int32_t batch, int32_t h, int32_t wdt, int32_t cin,
                                   int32_t cout, int32_t precision, void* stream) {
    EG_REQUIRE(dy && w_flip && dx && batch > 0 && h > 0 && wdt > 0, EG_ERR_BAD_ARG, "eg_conv3x3_dgrad_s2: null pointer or empty shape");
    EG_REQUIRE(precision == EG_PREC_BF16X3, EG_ERR_UNSUPPORTED, "eg_conv3x3_dgrad_s2: split-bf16 arithmetic only (precision %d)", precision);
    EG_REQUIRE(eg_aligned16(dy) && eg_aligned16(w_flip) && eg_aligned16(dx) && (!res_q || eg_aligned16(res_q)), EG_ERR_ALIGN,
               "eg_conv3x3_dgrad_s2: pointers must be 16-byte aligned");
    ConvArgs a;
    a.x = dy; a.w = w_flip; a.bias = nullptr; a.scale = nullptr; a.shift = nullptr; a.y = dx; a.gap = nullptr;
    a.H = (h - 1) / 2 + 1; a.W = (wdt - 1) / 2 + 1; a.Ho = h; a.Wo = wdt;          // the kernel's "input" is dy, its output dx
    a.cout = cin; a.relu = 0; a.nchw = 0; a.tiles_x = eg_cdiv(a.W, 32); a.tiles = 0;
    a.res_q = res_q;
    hipStream_t st = (hipStream_t)stream;
    EgProfScope prof((int64_t)cin * 1000000 + (int64_t)cout * 1000 + 200 + 8, 2.0 * 9 * cin * cout * (double)a.H * a.W * batch, st);
    if (cin == 32 && cout == 64) return launch_dgrad_s2<64, 2, 4, 4, 1>(a, batch, st);
    if (cin == 64 && cout == 128) return launch_dgrad_s2<128, 4, 2, 2, 2>(a, batch, st);
    if (cin == 128 && cout == 256) return launch_dgrad_s2<256, 8, 1, 1, 4>(a, batch, st);
    eg_set_error("eg_conv3x3_dgrad_s2: unsupported channels %d -> %d", cin, cout);
    return EG_ERR_UNSUPPORTED;
}

extern "C" int eg_stem_conv(const float* x, const float* w9xc, const float* bias, const float* scale, const float* shift,
                            float* y, int32_t batch, int32_t h, int32_t wdt, int32_t c, void* stream) {
    EG_REQUIRE(x && w9xc && bias && scale && shift && y && batch > 0, EG_ERR_BAD_ARG, "eg_stem_conv: null pointer");
    EG_REQUIRE(c % 4 == 0 && c <= 128 && 256 % (c / 4) == 0, EG_ERR_UNSUPPORTED, "eg_stem_conv: C=%d", c);
    // 256 % (C/4) == 0: a thread keeps its channel quad; one workgroup per output row
    hipLaunchKernelGGL(stem_conv_kernel, dim3(batch * h), dim3(256), 3 * (wdt + 2) * sizeof(float), (hipStream_t)stream, x, w9xc, bias, scale, shift, y,
                       batch, h, wdt, c);
    return eg_check_launch("stem_conv");
}

extern "C" int eg_se_gate(const float* gap_partial, int32_t tiles, const float* w1, const float* b1, const float* w2,
                          const float* b2, float* gate, int32_t batch, int32_t c, int32_t hw, void* stream) {
    EG_REQUIRE(gap_partial && w1 && b1 && w2 && b2 && gate && batch > 0, EG_ERR_BAD_ARG, "eg_se_gate: null pointer");
    EG_REQUIRE(c % 8 == 0 && c <= 256 && (c <= 128 ? 128 % c : 256 % c) == 0, EG_ERR_UNSUPPORTED, "eg_se_gate: C=%d", c);
    hipLaunchKernelGGL(se_gate_kernel, dim3(batch), dim3(c <= 128 ? 128 : 256), 0, (hipStream_t)stream, gap_partial, tiles, w1, b1, w2, b2,
                       gate, c, 1.0f / (float)hw);
    return eg_check_launch("se_gate");
}

namespace {
int se_gate_pre_launch(const float* t1, const float* gap_partial, int32_t tiles, const float* conv2_w, const float* scale2,
                       const float* shift2, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                       int32_t batch, int32_t h, int32_t wdt, int32_t c, void* stream, const float* ds_scale, const float* ds_shift, float* sc_vec) {
    EG_REQUIRE(t1 && gap_partial && conv2_w && scale2 && shift2 && w1 && b1 && w2 && b2 && gate && batch > 0 && h > 1 && wdt > 1, EG_ERR_BAD_ARG,
               "eg_se_gate_pre: null pointer or empty shape");
    EG_REQUIRE(c % 8 == 0 && c <= 256 && 256 % c == 0 && eg_aligned16(conv2_w), EG_ERR_UNSUPPORTED, "eg_se_gate_pre: C=%d", c);
    const size_t smem = sizeof(float) * (5 * GP_T + 9 * (size_t)c + GP_T + c + (c >> 3) + 4);
    EG_REQUIRE(!sc_vec || (ds_scale && ds_shift), EG_ERR_BAD_ARG, "eg_se_gate_pre: the shortcut vectors need the downsample BatchNorm");
    hipLaunchKernelGGL(se_gate_pre_kernel, dim3(batch), dim3(GP_T), smem, (hipStream_t)stream, t1, gap_partial, tiles, conv2_w, scale2, shift2, w1,
                       b1, w2, b2, gate, h, wdt, c, ds_scale, ds_shift, sc_vec);
    return eg_check_launch("se_gate_pre");
}
}  // namespace

extern "C" int eg_se_gate_pre(const float* t1, const float* gap_partial, int32_t tiles, const float* conv2_w, const float* scale2,
                              const float* shift2, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                              int32_t batch, int32_t h, int32_t wdt, int32_t c, void* stream) {
    return se_gate_pre_launch(t1, gap_partial, tiles, conv2_w, scale2, shift2, w1, b1, w2, b2, gate, batch, h, wdt, c, stream, nullptr, nullptr, nullptr);
}

// One SEBasicBlock (ResNetBlocks.py:21-37) in the audio tower's fused data flow, identity and stage-entry blocks alike (run_audio_tower calls this):
//   conv1 (stride s) -> ReLU -> BN1, with per-tile channel sums        t1, gap
//   gate from the moments of t1 (se_gate_pre_kernel)                    gate (+ the shortcut vectors f, q, h of a block with a downsample)
//   conv2 with the tail in its epilogue                                 out = relu(gate * BN2(conv2(t1)) + shortcut)
// ds_w == NULL: identity shortcut (cin == cout, stride 1), any precision.  ds_w != NULL: the 1x1 stride-s downsample's EG_PACK_CONV1X1_BF16 images, contracted
// inside conv2 (split-bf16 modes; 32 -> 64 and 64 -> 128).  Neither y nor the shortcut map exists; three launches.
extern "C" int eg_se_block_fused(const float* x, const float* conv1_w, const float* scale1, const float* shift1, const float* conv2_w, const float* scale2,
                                 const float* shift2, const float* se_w1, const float* se_b1, const float* se_w2, const float* se_b2, const float* ds_w,
                                 const float* ds_scale, const float* ds_shift, float* t1, float* out, float* gap_partial, float* gate, float* sc_vec,
                                 int32_t batch, int32_t h, int32_t wdt, int32_t cin, int32_t cout, int32_t stride, int32_t precision, void* stream) {
    EG_REQUIRE(x && conv1_w && scale1 && shift1 && conv2_w && scale2 && shift2 && t1 && out && gap_partial && gate, EG_ERR_BAD_ARG, "eg_se_block_fused: null pointer");
    EG_REQUIRE(ds_w ? (ds_scale && ds_shift && sc_vec) : (cin == cout && stride == 1), EG_ERR_BAD_ARG,
               "eg_se_block_fused: a downsample needs its BatchNorm and the shortcut vectors; an identity shortcut needs cin == cout and stride 1");
    EG_REQUIRE(stride == 1 || stride == 2, EG_ERR_UNSUPPORTED, "eg_se_block_fused: stride %d", stride);
    const int ho = (h + 2 - 3) / stride + 1, wo = (wdt + 2 - 3) / stride + 1;
    if (int rc = eg_conv3x3(x, conv1_w, nullptr, scale1, shift1, t1, gap_partial, batch, h, wdt, cin, cout, stride, 1, 0, precision, stream)) return rc;
    const int tiles1 = eg_conv3x3_gap_tiles(h, wdt, cin, cout, stride);
    if (int rc = se_gate_pre_launch(t1, gap_partial, tiles1, conv2_w, scale2, shift2, se_w1, se_b1, se_w2, se_b2, gate, batch, ho, wo, cout, stream,
                                    ds_w ? ds_scale : nullptr, ds_w ? ds_shift : nullptr, ds_w ? sc_vec : nullptr)) return rc;
    if (!ds_w) return eg_conv3x3_se(t1, conv2_w, nullptr, scale2, shift2, gate, x, out, nullptr, batch, ho, wo, cout, cout, 1, 0, 0, precision, stream);
    const ShortcutArgs sc{x, ds_w, sc_vec, h, wdt, cin, stride};
    return conv3x3_dispatch({.a = {.x = t1, .w = conv2_w, .y = out, .H = ho, .W = wo, .cout = cout},
                             .batch = batch, .cin = cout, .stride = 1, .precision = precision, .stream = stream, .sc = &sc});
}

extern "C" int eg_se_residual_relu(const float* y, const float* gate, const float* x_in, const float* ds_w,
                                   const float* ds_scale, const float* ds_shift, float* out, int32_t batch, int32_t ho,
                                   int32_t wo, int32_t c, int32_t h_in, int32_t w_in, int32_t cin, int32_t stride, void* stream) {
    EG_REQUIRE(y && gate && x_in && out && batch > 0, EG_ERR_BAD_ARG, "eg_se_residual_relu: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (!ds_w) {
        EG_REQUIRE(cin == c && h_in == ho && w_in == wo, EG_ERR_BAD_ARG, "eg_se_residual_relu: identity shortcut shape mismatch");
        const size_t n4 = (size_t)batch * ho * wo * c / 4;
        const int blocks = (int)((n4 + 255) / 256 < 8192 ? (n4 + 255) / 256 : 8192);
        hipLaunchKernelGGL(se_tail_identity_kernel, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const f4*>(y), gate,
                           reinterpret_cast<const f4*>(x_in), reinterpret_cast<f4*>(out), n4, ho * wo * (c / 4), c / 4);
        return eg_check_launch("se_tail");
    }
    EG_REQUIRE(ds_scale && ds_shift, EG_ERR_BAD_ARG, "eg_se_residual_relu: downsample BN missing");
    const size_t total = (size_t)batch * ho * wo * (c / 4);
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    if (cin == 32 && c == 64)
        hipLaunchKernelGGL((se_tail_downsample_kernel<32, 64>), dim3(blocks), dim3(256), 32 * 64 * 4, st, y, gate, x_in, ds_w, ds_scale,
                           ds_shift, out, batch, ho, wo, h_in, w_in, stride);
    else if (cin == 64 && c == 128)
        hipLaunchKernelGGL((se_tail_downsample_kernel<64, 128>), dim3(blocks), dim3(256), 64 * 128 * 4, st, y, gate, x_in, ds_w, ds_scale,
                           ds_shift, out, batch, ho, wo, h_in, w_in, stride);
    else if (cin == 128 && c == 256) {
        if (int rc = eg_ensure_dynamic_lds(reinterpret_cast<const void*>(se_tail_downsample_kernel<128, 256>), 128 * 256 * 4, "eg_se_residual_relu")) return rc;
        hipLaunchKernelGGL((se_tail_downsample_kernel<128, 256>), dim3(blocks < 1024 ? blocks : 1024), dim3(256), 128 * 256 * 4, st, y, gate,
                           x_in, ds_w, ds_scale, ds_shift, out, batch, ho, wo, h_in, w_in, stride);
    } else {
        eg_set_error("eg_se_residual_relu: unsupported downsample %d->%d", cin, c);
        return EG_ERR_UNSUPPORTED;
    }
    return eg_check_launch("se_tail_downsample");
}
