// Small kernels of the generator: LayerNorm, embedding gather, row-periodic add,
// TCN time-axis Linear, prior/memory encoder, CVAE conv1d / convT1d, reparameterise.
#include "common.h"
#include <stdlib.h>
#include <string.h>

namespace {

// ---- LayerNorm (Full_model/SubLayers.py:55-57,80-82): one wave per row, two-pass (corrected mean, then variance) in registers ----------
template <int NV>   // NV f4 per lane (D <= NV*256)
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                        const float* __restrict__ b, float* __restrict__ y, int rows, int D,
                                                        float eps, unsigned short* __restrict__ img) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const f4* xr = reinterpret_cast<const f4*>(x + (size_t)row * D);
    const int nq = D >> 2;
    f4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int q = lane + i * 64;
        v[i] = q < nq ? xr[q] : (f4){0.f, 0.f, 0.f, 0.f};
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    // The mean in two steps: the fp32 sum of D values carries an error of a few ulp of the mean, which 1 / sqrt(var + eps) multiplies (a constant
    // row: by 1e3, where the output should be beta).  The residuals x - m0 are small, so their sum corrects m0 to the rounding of the exact mean.
    const float m0 = wave_sum(s) / (float)D;
    float c = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int q = lane + i * 64;
        if (q < nq) {
            const f4 d = v[i] - m0;
            c += (d[0] + d[1]) + (d[2] + d[3]);
        }
    }
    const float mean = m0 + wave_sum(c) / (float)D;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int q = lane + i * 64;
        if (q < nq) {
            const f4 d = v[i] - mean;
            ss += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)D + eps);
    f4* yr = reinterpret_cast<f4*>(y + (size_t)row * D);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int q = lane + i * 64;
        if (q < nq) {
            const f4 o = (v[i] - mean) * rstd * reinterpret_cast<const f4*>(g)[q] + reinterpret_cast<const f4*>(b)[q];
            yr[q] = o;
            if (img) {      // also emit the row as bf16 (hi, lo) tile-planar images for the products that consume it
                const f4 z = (f4){0.f, 0.f, 0.f, 0.f};
                bf8 h8, l8;
                split_octet<true>(o, z, h8, l8);
                const int KO = D >> 3;
                const size_t slot = (((size_t)(row >> 6) * KO + (q >> 1)) * 64 + (row & 63)) * 8 + (q & 1) * 4;
                const size_t lo_off = (size_t)((rows + 63) >> 6) * KO * 512;
                typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
                const u32x4_t hh = __builtin_bit_cast(u32x4_t, h8), ll = __builtin_bit_cast(u32x4_t, l8);
                *reinterpret_cast<u32x2*>(img + slot) = (u32x2){hh[0], hh[1]};
                *reinterpret_cast<u32x2*>(img + lo_off + slot) = (u32x2){ll[0], ll[1]};
            }
        }
    }
}

// any D (rows not 16-byte aligned, e.g. the 282-wide encoder of Pose_Discriminator, Models_spatial_memory.py:671-704): scalar accesses, same two-pass order
__global__ __launch_bounds__(256) void layernorm_any_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
                                                            float* __restrict__ y, int rows, int D, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (size_t)row * D;
    float s = 0.f;
    for (int i = lane; i < D; i += 64) s += xr[i];
    const float m0 = wave_sum(s) / (float)D;
    float c = 0.f;
    for (int i = lane; i < D; i += 64) c += xr[i] - m0;
    const float mean = m0 + wave_sum(c) / (float)D;            // two-step mean, as in layernorm_kernel
    float ss = 0.f;
    for (int i = lane; i < D; i += 64) { const float d = xr[i] - mean; ss += d * d; }
    const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)D + eps);
    for (int i = lane; i < D; i += 64) y[(size_t)row * D + i] = (xr[i] - mean) * rstd * g[i] + b[i];
}

__global__ __launch_bounds__(256) void add_rows_any_kernel(const float* __restrict__ a, const float* __restrict__ table, float* __restrict__ out,
                                                           size_t n, int d, int period) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t row = i / d;
        const size_t trow = period > 0 ? row % period : row;
        out[i] = a[i] + table[trow * d + (i - row * d)];
    }
}

// ---- elementwise helpers -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void embedding_kernel(const int64_t* __restrict__ idx, const float* __restrict__ table,
                                                        float* __restrict__ out, int rows, int dim, int ld, int n_words) {
    const int dq = dim >> 2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)rows * dq; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i / dq), c = (int)(i % dq);
        int64_t w = idx[r];
        w = w < 0 ? 0 : (w >= n_words ? n_words - 1 : w);
        *reinterpret_cast<f4*>(out + (size_t)r * ld + c * 4) = *reinterpret_cast<const f4*>(table + (size_t)w * dim + c * 4);
    }
}

// The same rows with their bf16 (hi, lo) tile-planar images [ceil(rows/64)][ld/8][64][8] for a pre-split product (ld = dim rounded up to 64): one
// thread per (row, octet); the columns dim .. ld-1 are written as zeros in the fp32 rows and in the images.  zero (optional): a line of 64 * ld / 8
// slots this launch clears -- the row source of the causal products that follow on the stream (t < dilation).
__global__ __launch_bounds__(256) void embedding_img_kernel(const int64_t* __restrict__ idx, const float* __restrict__ table, float* __restrict__ out,
                                                            bf8* __restrict__ hi, bf8* __restrict__ lo, bf8* __restrict__ zero, int rows, int dim, int ld,
                                                            int n_words) {
    const int KO = ld >> 3;
    const size_t total = (size_t)((rows + 63) >> 6) * 64 * KO;            // consecutive threads = consecutive rows of one octet: 1-KiB image stores
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        if (zero && i < (size_t)64 * KO) zero[i] = (bf8){0, 0, 0, 0, 0, 0, 0, 0};
        const int t = (int)(i / (64 * KO)), rem = (int)(i - (size_t)t * 64 * KO), o = rem >> 6, r = t * 64 + (rem & 63), k = o * 8;
        if (r >= rows) continue;
        int64_t w = idx[r];
        w = w < 0 ? 0 : (w >= n_words ? n_words - 1 : w);
        f4 v0 = (f4){0.f, 0.f, 0.f, 0.f}, v1 = v0;
        if (k < dim) v0 = *reinterpret_cast<const f4*>(table + (size_t)w * dim + k);
        if (k + 4 < dim) v1 = *reinterpret_cast<const f4*>(table + (size_t)w * dim + k + 4);
        *reinterpret_cast<f4*>(out + (size_t)r * ld + k) = v0;
        *reinterpret_cast<f4*>(out + (size_t)r * ld + k + 4) = v1;
        bf8 h, l;
        split_octet<true>(v0, v1, h, l);
        const size_t slot = ((size_t)(r >> 6) * KO + o) * 64 + (r & 63);
        hi[slot] = h;
        lo[slot] = l;
    }
}

// out = a + b ;  b optionally row-periodic (row % period) -- positional table add (Models_spatial_memory.py:46-48)
__global__ __launch_bounds__(256) void add_kernel(const f4* __restrict__ a, const f4* __restrict__ b, f4* __restrict__ out,
                                                  size_t n4, int row_q, int period) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        size_t j = i;
        if (period) {
            const size_t row = i / row_q;
            j = (row % period) * row_q + (i - row * row_q);
        }
        out[i] = a[i] + b[j];
    }
}

// add_kernel with a second output: the sum split to bf16 (hi, lo) tile-planar images [ceil(rows/64)][row_len/8][64][8] for a pre-split product.
// One thread per (row, octet), consecutive threads = consecutive rows of one octet (1-KiB image stores); row_o = row_len / 8.
__global__ __launch_bounds__(256) void add_img_kernel(const f4* __restrict__ a, const f4* __restrict__ b, f4* __restrict__ out, bf8* __restrict__ hi,
                                                      bf8* __restrict__ lo, size_t rows, int row_o, int period) {
    const size_t total = ((rows + 63) >> 6) * 64 * row_o;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        const size_t tile = t / (64 * (size_t)row_o);
        const int rem = (int)(t - tile * 64 * row_o), o = rem >> 6;
        const size_t row = tile * 64 + (rem & 63);
        if (row >= rows) continue;
        const size_t i = row * row_o + o;
        const size_t j = period ? (row % period) * row_o + o : i;
        const f4 v0 = a[2 * i] + b[2 * j], v1 = a[2 * i + 1] + b[2 * j + 1];
        out[2 * i] = v0;
        out[2 * i + 1] = v1;
        bf8 h, l;
        split_octet<true>(v0, v1, h, l);
        const size_t slot = ((row >> 6) * row_o + o) * 64 + (row & 63);
        hi[slot] = h;
        lo[slot] = l;
    }
}

// ---- TextEncoderTCN.fc1: Linear over the time axis (Models_spatial_memory.py:164-166,176) -----------------
// x, y [B, L, C] channels-last:  y[b,t',c] = bias[t'] + sum_t W[t',t] x[b,t,c]
// Reference form (EG_TIME_LINEAR=ref, this round's A/B and bit-equality reference): W and x in LDS, one output row at a time, two LDS reads
// per multiply-add.
__global__ __launch_bounds__(256) void time_linear_ref_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ y, int L, int C, int ld) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Ws = sm;             // [L][L]
    float* Xs = sm + L * L;     // [L][64]
    const int b = blockIdx.y, c0 = blockIdx.x * 64, tid = threadIdx.x;
    for (int i = tid; i < L * L; i += 256) Ws[i] = w[i];
    for (int i = tid; i < L * 64; i += 256) {
        const int t = i >> 6, c = i & 63;
        Xs[i] = (c0 + c < C) ? x[((size_t)b * L + t) * ld + c0 + c] : 0.f;
    }
    __syncthreads();
    const int c = tid & 63;
    if (c0 + c >= C) return;
    for (int tp = tid >> 6; tp < L; tp += 4) {
        float s = bias[tp];
        for (int t = 0; t < L; ++t) s += Ws[tp * L + t] * Xs[t * 64 + c];
        y[((size_t)b * L + tp) * ld + c0 + c] = s;
    }
}

// R output rows tp0, tp0 + 4, ... of one wave, accumulated together: per four values of t a thread reads four x values (one LDS read each,
// serving R multiply-adds apiece) and R weight quads, each ONE 16-byte LDS read whose address is the same in every lane (tp0 is wave-uniform: a
// broadcast, 4 LDS cycles for 4 R multiply-adds).  Per output element the sum is the reference kernel's: bias first, then t ascending, one
// multiply-add per term -- bit-equal.  Ws rows are Lp = round_up(L, 4) floats apart, so every quad is 16-byte aligned.
template <int R>
__device__ __forceinline__ void time_linear_rows(const float* Ws, const float* Xs, const float* __restrict__ bias, float* __restrict__ yc, int tp0,
                                                 int L, int Lp, int ld, int c) {
    float acc[R];
#pragma unroll
    for (int k = 0; k < R; ++k) acc[k] = bias[tp0 + 4 * k];
    const float* wr = Ws + tp0 * Lp;
    const int L4 = L & ~3;
    int t = 0;
#pragma unroll 2
    for (; t < L4; t += 4) {
        float xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) xv[u] = Xs[(t + u) * 64 + c];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const f4 wv = *reinterpret_cast<const f4*>(wr + 4 * k * Lp + t);
            acc[k] += wv.x * xv[0];
            acc[k] += wv.y * xv[1];
            acc[k] += wv.z * xv[2];
            acc[k] += wv.w * xv[3];
        }
    }
    for (; t < L; ++t) {
        const float xv = Xs[t * 64 + c];
#pragma unroll
        for (int k = 0; k < R; ++k) acc[k] += wr[4 * k * Lp + t] * xv;
    }
#pragma unroll
    for (int k = 0; k < R; ++k) yc[(size_t)(tp0 + 4 * k) * ld] = acc[k];
}

// Same grid and row ownership as the reference form (64 channels x clip per workgroup; wave v owns rows v, v + 4, ...).  A thread keeps its rows'
// sums in registers, fifteen at a time (L = 60: all of a wave's rows in one walk over t), then five, then one, so any L works.  W and x are staged
// with up to 32 loads in flight per thread (the reference form's one-at-a-time copy loop pays a memory latency per element).
__global__ __launch_bounds__(256) void time_linear_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ y, int L, int C, int ld) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int Lp = (L + 3) & ~3;
    float* Ws = sm;             // [L][Lp]
    float* Xs = sm + L * Lp;    // [L][64]
    const int b = blockIdx.y, c0 = blockIdx.x * 64, tid = threadIdx.x, c = tid & 63;
    const bool live = c0 + c < C;
    const float* xc = x + (size_t)b * L * ld + c0 + c;
    for (int i0 = tid; i0 < L * max(L, 64); i0 += 16 * 256) {
        float vx[16], vw[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int i = i0 + u * 256;
            vx[u] = (live && i < L * 64) ? xc[(size_t)(i >> 6) * ld] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int i = i0 + u * 256;
            vw[u] = i < L * L ? w[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int i = i0 + u * 256;
            if (i < L * 64) Xs[i] = vx[u];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int i = i0 + u * 256, r = i / L;
            if (i < L * L) Ws[r * Lp + (i - r * L)] = vw[u];
        }
    }
    __syncthreads();
    int tp = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (!live) return;
    float* yc = y + (size_t)b * L * ld + c0 + c;
    for (; tp + 56 < L; tp += 60) time_linear_rows<15>(Ws, Xs, bias, yc, tp, L, Lp, ld, c);
    for (; tp + 16 < L; tp += 20) time_linear_rows<5>(Ws, Xs, bias, yc, tp, L, Lp, ld, c);
    for (; tp < L; tp += 4) time_linear_rows<1>(Ws, Xs, bias, yc, tp, L, Lp, ld, c);
}

// ---- Prior_MemoryEncoder front half (Models_spatial_memory.py:366-390; Models_memory.py:233-251,282-287) ---
struct PriorArgs {
    const float* prior;         // [B,P,D]
    const float *w1, *b1, *s1, *t1;     // Conv1d(P->PL,k3) raw [PL][P][3], bias, BN scale/shift
    const float *w2, *b2, *s2, *t2;     // Conv1d(PL->PL,k3)
    // memory variant (NULL for spatial): SP_v1 chunk encoder and TM encoders, raw nn.Linear layouts
    const float *sp_w0, *sp_b0, *sp_w1, *sp_b1;         // [D, chunk*D], [D], [D,D], [D]
    const float *tc_w0, *tc_b0, *tc_w1, *tc_b1;         // temporal_chunk_encoder
    const float *tm_w0, *tm_b0, *tm_w1, *tm_b1;         // temporal_memory_encoder [chunk, chunk*D], [chunk], [chunk,chunk], [chunk]
    float* cat;                 // [B,F,Dpad] = cat(prior, pred), zero padded
    float* tm_mem;              // [B,D]
    float* tm_pe;               // [B,chunk]
    int P, PL, D, Dpad, chunk, variant, stage_w, dchunk;
};

__device__ __forceinline__ float block_dot(const float* __restrict__ wrow, const float* __restrict__ xs, int n, int lane) {
    float s = 0.f;
    for (int i = lane; i < n; i += 64) s += wrow[i] * xs[i];
    return wave_sum(s);
}

__global__ __launch_bounds__(256) void prior_pred_kernel(PriorArgs a) {
    // one workgroup = (clip, slice [d0, d0+dc) of the pose axis); the two stacked k=3 convs need a halo of 2 on the input and
    // 1 on the hidden map.  The memory variant (SP_v1 / TM need whole-row inner products) runs with one slice = the whole axis.
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int P = a.P, PL = a.PL, D = a.D;
    const int d0 = blockIdx.y * a.dchunk, dc = min(a.dchunk, D - d0);
    const int XW = dc + 4, HW = dc + 2;
    float* xs = sm;                     // [P][dc+4]   x[d0-2 .. d0+dc+1], zero outside [0, D)
    float* h1 = xs + P * XW;            // [PL][dc+2]  hidden[d0-1 .. d0+dc], zero outside [0, D) (conv2's padding)
    float* h2 = h1 + PL * HW;           // [PL][dc]
    float* v0 = h2 + PL * dc;           // [chunk*D] flat chunk / scratch (memory variant)
    float* v1 = v0 + (a.variant == 1 ? a.chunk * D : 0);
    float* v2 = v1 + (a.variant == 1 ? D : 0);
    float* w1s = v2 + (a.variant == 1 ? D : 0);         // conv weights staged once when they fit
    float* w2s = w1s + PL * P * 3;
    if (a.stage_w) {
        for (int i = tid; i < PL * P * 3; i += 256) w1s[i] = a.w1[i];
        for (int i = tid; i < PL * PL * 3; i += 256) w2s[i] = a.w2[i];
    }
    const float* w1p = a.stage_w ? w1s : a.w1;
    const float* w2p = a.stage_w ? w2s : a.w2;
    for (int i = tid; i < P * XW; i += 256) {
        const int f = i / XW, d = d0 - 2 + (i - f * XW);
        xs[i] = (d >= 0 && d < D) ? a.prior[((size_t)b * P + f) * D + d] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < PL * HW; i += 256) {
        const int co = i / HW, j = i - co * HW, d = d0 - 1 + j;
        float v = 0.f;
        if (d >= 0 && d < D) {
            float s = a.b1[co];
            for (int ci = 0; ci < P; ++ci) {
                const float* wp = w1p + (co * P + ci) * 3;
                const float* xp = xs + ci * XW + j;           // x[d-1], x[d], x[d+1]
                s += wp[0] * xp[0] + wp[1] * xp[1] + wp[2] * xp[2];
            }
            v = fmaxf(s, 0.f) * a.s1[co] + a.t1[co];
        }
        h1[i] = v;
    }
    __syncthreads();
    for (int i = tid; i < PL * dc; i += 256) {
        const int co = i / dc, j = i - co * dc;
        float s = a.b2[co];
        for (int ci = 0; ci < PL; ++ci) {
            const float* wp = w2p + (co * PL + ci) * 3;
            const float* xp = h1 + ci * HW + j;               // hidden[d-1], [d], [d+1]
            s += wp[0] * xp[0] + wp[1] * xp[1] + wp[2] * xp[2];
        }
        h2[i] = fmaxf(s, 0.f) * a.s2[co] + a.t2[co];
    }
    __syncthreads();
    if (a.variant == 1) {               // d0 == 0, dc == D here
        const int CD = a.chunk * D;
        for (int i = tid; i < CD; i += 256) {               // flat last-chunk prior frames (Models_memory.py:237)
            const int f = i / D, d = i - f * D;
            v0[i] = xs[(P - a.chunk + f) * XW + d + 2];
        }
        __syncthreads();
        // SP_v1: mem = L1(L0(flat)) ; s = sigmoid(<mem, pred_c>) ; pred_c = s*pred_c + (1-s)*mem
        for (int n = wave; n < D; n += 4) {
            const float s = block_dot(a.sp_w0 + (size_t)n * CD, v0, CD, lane);
            if (lane == 0) v1[n] = s + a.sp_b0[n];
        }
        __syncthreads();
        for (int n = wave; n < D; n += 4) {
            const float s = block_dot(a.sp_w1 + (size_t)n * D, v1, D, lane);
            if (lane == 0) v2[n] = s + a.sp_b1[n];
        }
        __syncthreads();
        // TM memory encoding uses the same flat chunk (Models_memory.py:285): compute before v1 is reused
        for (int n = wave; n < D; n += 4) {
            const float s = block_dot(a.tc_w0 + (size_t)n * CD, v0, CD, lane);
            if (lane == 0) v1[n] = s + a.tc_b0[n];
        }
        __syncthreads();
        for (int n = wave; n < D; n += 4) {
            const float s = block_dot(a.tc_w1 + (size_t)n * D, v1, D, lane);
            if (lane == 0) a.tm_mem[(size_t)b * D + n] = s + a.tc_b1[n];
        }
        for (int c = wave; c < a.chunk; c += 4) {           // gate each of the first `chunk` predicted frames
            const float dot = block_dot(v2, h2 + c * D, D, lane);
            const float sg = 1.f / (1.f + expf(-dot));
            for (int d = lane; d < D; d += 64) h2[c * D + d] = sg * h2[c * D + d] + (1.f - sg) * v2[d];
        }
        __syncthreads();
        // TM pred encoding on the gated frames: pe = M1(M0(flat(pred[:chunk])))  (Models_memory.py:286)
        for (int n = wave; n < a.chunk; n += 4) {
            const float s = block_dot(a.tm_w0 + (size_t)n * CD, h2, CD, lane);
            if (lane == 0) v1[n] = s + a.tm_b0[n];
        }
        __syncthreads();
        if (tid < a.chunk) {
            float s = a.tm_b1[tid];
            for (int j = 0; j < a.chunk; ++j) s += a.tm_w1[tid * a.chunk + j] * v1[j];
            a.tm_pe[(size_t)b * a.chunk + tid] = s;
        }
    }
    // cat(prior, pred) rows for this slice; the last slice also zeroes the pad columns [D, Dpad)
    const int F = P + PL;
    const int dend = (d0 + dc >= D) ? a.Dpad : d0 + dc, wcols = dend - d0;
    for (int i = tid; i < F * wcols; i += 256) {
        const int f = i / wcols, d = d0 + (i - f * wcols);
        float v = 0.f;
        if (d < D) v = f < P ? xs[f * XW + (d - d0) + 2] : h2[(f - P) * dc + (d - d0)];
        a.cat[((size_t)b * F + f) * a.Dpad + d] = v;
    }
}

// TM_Memory_Net cross-batch step (Models_memory.py:288-292):  G = mem^T @ pe  [D,chunk]  (sum over the batch)
__global__ __launch_bounds__(256) void tm_gram_kernel(const float* __restrict__ mem, const float* __restrict__ pe,
                                                      float* __restrict__ G, int B, int D, int chunk) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= D * chunk) return;
    const int d = i / chunk, c = i - d * chunk;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += mem[(size_t)b * D + d] * pe[(size_t)b * chunk + c];
    G[i] = s;
}
// score = mem[b] @ G ; w = softmax(score) ; cat[b, P+c, :] *= (1 + w[c])
__global__ __launch_bounds__(64) void tm_apply_kernel(const float* __restrict__ mem, const float* __restrict__ G,
                                                      float* __restrict__ cat, int D, int Dpad, int chunk, int P, int F) {
    __shared__ float sc[64];
    const int b = blockIdx.x, lane = threadIdx.x;
    float mx = -3.0e38f;
    for (int c = 0; c < chunk; ++c) {
        float s = 0.f;
        for (int d = lane; d < D; d += 64) s += mem[(size_t)b * D + d] * G[d * chunk + c];
        s = wave_sum(s);
        if (lane == 0) sc[c] = s;
        mx = fmaxf(mx, s);
    }
    __syncthreads();
    float den = 0.f;
    for (int c = 0; c < chunk; ++c) den += expf(sc[c] - mx);
    for (int c = 0; c < chunk; ++c) {
        const float w = expf(sc[c] - mx) / den;
        float* row = cat + ((size_t)b * F + P + c) * Dpad;
        for (int d = lane; d < D; d += 64) row[d] = row[d] + row[d] * w;
    }
}

// ---- CVAE 1-D convolutions (CAVE/BEAT_CVAE.py:318-332,355-369), layout [n][C][L] ----------------------------
// y[n,co,l] = post( bias[co] + sum_{ci,k} w[co,ci,k] x[n,ci,l*stride + k - pad] );  post = LeakyReLU(0.2) (act) then BN affine (scale != NULL)
// One workgroup = (sample, 64 output positions, 4*COG output channels): the input tile lives in LDS, each wave owns
// COG output channels (wave-uniform => the weight reads are scalar loads) accumulated in registers, so every LDS read of
// x is reused COG times.
template <int COG>
__global__ __launch_bounds__(256) void conv1d_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, const float* __restrict__ scale,
                                                     const float* __restrict__ shift, float* __restrict__ y, int Cin, int Cout,
                                                     int Lin, int Lout, int K, int stride, int pad, int act) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int n = blockIdx.y, l0 = blockIdx.x * 64, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int span = 63 * stride + K;
    const int in0 = l0 * stride - pad;
    const int cblk = 4 * COG;                        // output channels of this workgroup
    const int cbase = blockIdx.z * cblk;
    float* xs = sm;                                 // [Cin][span]
    float* ws = sm + ((Cin * span + 3) & ~3);       // [Cin*K][cblk]: the COG weights of a wave are COG/4 broadcast b128 reads
    for (int i = tid; i < Cin * span; i += 256) {
        const int ci = i / span, j = i - ci * span, gl = in0 + j;
        xs[i] = (gl >= 0 && gl < Lin) ? x[((size_t)n * Cin + ci) * Lin + gl] : 0.f;
    }
    for (int i = tid; i < Cin * K * cblk; i += 256) {
        const int ck = i / cblk, c = i - ck * cblk, co = cbase + c;
        ws[i] = co < Cout ? w[(size_t)co * Cin * K + ck] : 0.f;
    }
    __syncthreads();
    const int co0 = cbase + wave * COG;
    const int l = l0 + lane;
    f4 acc[COG / 4];
#pragma unroll
    for (int j = 0; j < COG / 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[j][r] = (co0 + j * 4 + r < Cout) ? bias[co0 + j * 4 + r] : 0.f;
    for (int ci = 0; ci < Cin; ++ci) {
        const float* xp = xs + ci * span + lane * stride;
        for (int k = 0; k < K; ++k) {
            const float xv = xp[k];
            const f4* wp = reinterpret_cast<const f4*>(ws + (ci * K + k) * cblk + wave * COG);
#pragma unroll
            for (int j = 0; j < COG / 4; ++j) acc[j] += wp[j] * xv;
        }
    }
    if (l >= Lout) return;
#pragma unroll
    for (int j = 0; j < COG / 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = co0 + j * 4 + r;
            if (co < Cout) {
                float s = acc[j][r];
                if (act) s = s > 0.f ? s : 0.2f * s;
                if (scale) s = s * scale[co] + shift[co];      // the affine does not depend on act
                y[((size_t)n * Cout + co) * Lout + l] = s;
            }
        }
}

// ConvTranspose1d(k=3, stride=2, padding=1, output_padding=1): Lout = 2*Lin; weight [Cin][Cout][3]
// y[co, lo] = bias + sum_ci sum_k [ (lo + 1 - k) even, li = (lo+1-k)/2 in range ] x[ci, li] w[ci, co, k]
// Left as the serial per-term walk it was: eg_cvae_sample no longer comes here (cvae_sample_fused_kernel below), only the training-mode forward
// and the frames = 120 fall-back do, and its term order is the one the fused kernel reproduces.
__global__ __launch_bounds__(128) void convt1d_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, float* __restrict__ y, int Cin, int Cout,
                                                      int Lin) {
    const int n = blockIdx.y, lo = blockIdx.x * 128 + threadIdx.x, Lout = 2 * Lin;
    if (lo >= Lout) return;
    for (int co = 0; co < Cout; ++co) {
        float s = bias[co];
        for (int ci = 0; ci < Cin; ++ci) {
            const float* xr = x + ((size_t)n * Cin + ci) * Lin;
            const float* wr = w + ((size_t)ci * Cout + co) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int t = lo + 1 - k;
                if (t >= 0 && !(t & 1) && (t >> 1) < Lin) s += xr[t >> 1] * wr[k];
            }
        }
        s = s > 0.f ? s : 0.2f * s;
        s = s * scale[co] + shift[co];
        y[((size_t)n * Cout + co) * Lout + lo] = s;
    }
}

// tiny dense layer for the CVAE MLPs (<= 512 wide): y[n, o] = bias[o] + sum_i w[o,i] x[n,i]; one wave per output
__global__ __launch_bounds__(256) void small_linear_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ y, int ldy,
                                                           int In, int Out) {
    const int n = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int o = blockIdx.x * 4 + wave; o < Out; o += gridDim.x * 4) {
        float s = 0.f;
        for (int i = lane; i < In; i += 64) s += w[(size_t)o * In + i] * x[(size_t)n * ldx + i];
        s = wave_sum(s);
        if (lane == 0) y[(size_t)n * ldy + o] = s + bias[o];
    }
}

__global__ __launch_bounds__(256) void reparam_kernel(const float* __restrict__ mu, const float* __restrict__ logvar,
                                                      const float* __restrict__ eps, float* __restrict__ z, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) z[i] = eps[i] * expf(0.5f * logvar[i]) + mu[i];
}

__global__ __launch_bounds__(256) void copy2d_kernel(const float* __restrict__ src, int lds_, float* __restrict__ dst, int ldd,
                                                     int rows, int cols) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)rows * cols; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i / cols), c = (int)(i % cols);
        dst[(size_t)r * ldd + c] = src[(size_t)r * lds_ + c];
    }
}

// ---- CVAE sample, fused: Posterior_Y_embedding -> fusion_z_posterior -> Decoder (BEAT_CVAE.py:355-369,440-446) in one launch ----------
// One workgroup = (sample n, tile [l0, l0 + T) of the L = d_model axis).  It recomputes the MLP head, then walks the five decoder stages for
// its tile with every intermediate in LDS; each stage also produces the halo the next one reads:
//   out [l0, l0+T)  <-  d4 [l0-1, l0+T+1)  <-  d3 [l0-2, l0+T+2)  <-  d2 [l0-4, l0+T+4)  <-  d1 [l0/2-2, l0/2+T/2+4)  <-  z0 [l0/4-1, l0/4+T/4+3)
// (d2 / d1 start on an even position so that a transposed stage is a walk over input positions li: output 2*li takes the tap k = 1 of x[li],
// output 2*li + 1 the taps k = 0 of x[li + 1] and k = 2 of x[li] -- no per-term parity branch; T % 4 == 0 keeps l0/2 - 2 even).  A position
// outside [0, L_stage) is the next stage's zero padding and is stored as 0, never computed from the bias; that zero is also what drops the
// tap li + 1 == Lin of the last odd output (the chain skips that term, here it is + 0 * w: the same value unless the accumulator is exactly -0
// or the weight is not finite).  Every output element is summed in the order of the launch chain it replaces (small_linear_kernel,
// convt1d_kernel, conv1d_kernel: bias first, ci outer, k inner, LeakyReLU, then the BatchNorm affine), so the result is the chain's bit for bit.
constexpr int CVAE_WAVES = 8;       // two waves per SIMD: one wave's LDS reads run under the other's FMAs
struct CvaeFusedLds {       // float offsets into the dynamic LDS; d4 overlays the buffers that are dead once d3 is complete
    int n0, n1, n2, n3, n4, cbF, d3, w6, w7, head, z0, d1, d2, w5, d4, total;
};
__host__ __device__ inline CvaeFusedLds cvae_fused_lds(int F, int T) {
    CvaeFusedLds s;
    s.n0 = T / 4 + 4; s.n1 = T / 2 + 6; s.n2 = T + 8; s.n3 = T + 4; s.n4 = T + 2;
    s.cbF = (F + 7) & ~7;                            // output channels in groups of 8: the row length of the staged F-wide weights
    int o = 0;
    s.d3 = o; o += (32 * s.n3 + 3) & ~3;
    s.w6 = o; o += 32 * 3 * s.cbF;
    s.w7 = o; o += F * 3 * s.cbF;
    s.d4 = o;
    s.head = o; o += 16 + 64 + 128;                  // py_h | zy = [z | post_y] | fz_h
    s.z0 = o; o += 4 * s.n0;
    s.d1 = o; o += (8 * s.n1 + 3) & ~3;
    s.d2 = o; o += 16 * s.n2;
    s.w5 = o; o += 16 * 3 * 32;
    const int d4_end = s.d4 + ((F * s.n4 + 3) & ~3);
    s.total = o > d4_end ? o : d4_end;
    return s;
}

// conv weights [Cout][CK] -> LDS [CK][CB] (zero beyond Cout), the layout conv1d_kernel stages
__device__ __forceinline__ void cvae_stage_w(float* __restrict__ dst, const float* __restrict__ w, int Cout, int CK, int CB, int tid) {
    for (int i = tid; i < CK * CB; i += 64 * CVAE_WAVES) {
        const int ck = i / CB, c = i - ck * CB;
        dst[i] = c < Cout ? w[(size_t)c * CK + ck] : 0.f;
    }
}

// y[o] = bias[o] + sum_i w[o][i] x[i], one wave per output exactly as small_linear_kernel sums it; R outputs of a wave in flight at a time
template <int R>
__device__ __forceinline__ void cvae_linear(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                            float* __restrict__ y, int In, int Out, int wave, int lane) {
    for (int o0 = wave * R; o0 < Out; o0 += CVAE_WAVES * R) {
        float t[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int o = o0 + r;
            float s = 0.f;
            if (o < Out)
                for (int i = lane; i < In; i += 64) s += w[(size_t)o * In + i] * x[i];
            t[r] = s;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) t[r] = wave_sum(t[r]);
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (o0 + r < Out) y[o0 + r] = t[r] + bias[o0 + r];
        }
    }
}

// ConvTranspose1d(k 3, stride 2, pad 1, output pad 1) + LeakyReLU + affine, LDS -> LDS.  xin [Cin][nin] and yout [Cout][nout] start at
// positions p and 2p (pos0 = 2p); a lane owns the input position j and its two outputs, a wave COG output channels (wave-uniform weights).
template <int COG>
__device__ __forceinline__ void cvae_convt_stage(const float* __restrict__ xin, int nin, const float* __restrict__ w,
                                                 const float* __restrict__ bias, const float* __restrict__ scale,
                                                 const float* __restrict__ shift, float* __restrict__ yout, int nout, int Cin, int Cout,
                                                 int pos0, int Lout, int wave, int lane) {
    const int npairs = nout >> 1, ng = Cout / COG, nitems = ng * ((npairs + 63) >> 6);
    for (int item = wave; item < nitems; item += CVAE_WAVES) {
        const int g = item % ng, j = (item / ng) * 64 + lane;
        if (j >= npairs) continue;
        float e[COG], o[COG];
#pragma unroll
        for (int r = 0; r < COG; ++r) e[r] = o[r] = bias[g * COG + r];
        for (int ci = 0; ci < Cin; ++ci) {
            const float x0 = xin[ci * nin + j], x1 = xin[ci * nin + j + 1];
#pragma unroll
            for (int r = 0; r < COG; ++r) {
                const float* wr = w + ((size_t)ci * Cout + g * COG + r) * 3;
                o[r] += x1 * wr[0];
                e[r] += x0 * wr[1];
                o[r] += x0 * wr[2];
            }
        }
        const int pe = pos0 + 2 * j;
        const bool in_e = pe >= 0 && pe < Lout, in_o = pe + 1 >= 0 && pe + 1 < Lout;
#pragma unroll
        for (int r = 0; r < COG; ++r) {
            const int co = g * COG + r;
            float se = e[r], so = o[r];
            se = se > 0.f ? se : 0.2f * se;
            so = so > 0.f ? so : 0.2f * so;
            se = se * scale[co] + shift[co];
            so = so * scale[co] + shift[co];
            yout[co * nout + 2 * j] = in_e ? se : 0.f;
            yout[co * nout + 2 * j + 1] = in_o ? so : 0.f;
        }
    }
}

// Conv1d(k 3, pad 1) with conv1d_kernel's inner loop: a wave owns 8 output channels (f4 broadcast reads of the staged weights), a lane a position,
// every LDS read of x feeds 8 FMAs.  xin [Cin][nin]: output index p reads xin[xoff + p + k].  FINAL: plain, to out[co][pos0 + p] in global
// memory where pos0 + p < L; otherwise LeakyReLU + affine to yout [Cout][nout] in LDS, zero outside [0, L).
template <bool FINAL>
__device__ __forceinline__ void cvae_conv_stage(const float* __restrict__ xin, int nin, int xoff, const float* __restrict__ wl, int CB,
                                                const float* __restrict__ bias, const float* __restrict__ scale,
                                                const float* __restrict__ shift, float* __restrict__ yout, int nout, int Cin, int Cout,
                                                int pos0, int L, int wave, int lane) {
    const int ng = CB >> 3, nitems = ng * ((nout + 63) >> 6);
    for (int item = wave; item < nitems; item += CVAE_WAVES) {
        const int g = item % ng, p = (item / ng) * 64 + lane;
        const int co0 = g * 8;
        f4 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[j][r] = (co0 + j * 4 + r < Cout) ? bias[co0 + j * 4 + r] : 0.f;
        const float* xp = xin + xoff + (p < nout ? p : nout - 1);        // lanes past the stage's span read its last position and store nothing
        const float* wg = wl + co0;
#pragma unroll 4
        for (int ci = 0; ci < Cin; ++ci) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float xv = xp[ci * nin + k];
                const f4* wp = reinterpret_cast<const f4*>(wg + (ci * 3 + k) * CB);
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] += wp[j] * xv;
            }
        }
        if (p >= nout) continue;
        const int pos = pos0 + p;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + j * 4 + r;
                if (co < Cout) {
                    float s = acc[j][r];
                    if (FINAL) {
                        if (pos < L) yout[(size_t)co * L + pos] = s;
                    } else {
                        s = s > 0.f ? s : 0.2f * s;
                        s = s * scale[co] + shift[co];
                        yout[co * nout + p] = (pos >= 0 && pos < L) ? s : 0.f;
                    }
                }
            }
    }
}

__global__ __launch_bounds__(64 * CVAE_WAVES) void cvae_sample_fused_kernel(const EgiCvaeFused a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int F = a.F, L = a.L, T = a.T, l0 = blockIdx.x * T;
    const CvaeFusedLds s = cvae_fused_lds(F, T);
    // The head's two wide layers (fz0: 128 x 64, the tile's rows of fz2: up to 144 x 128) are one global-memory latency each if fetched when
    // their input is ready; the rows a wave sums depend on l0 alone, so their weights and biases are fetched here, before anything else.
    constexpr int FR = 128 / CVAE_WAVES, ZR = 18;               // outputs per wave; 4 * n0 <= CVAE_WAVES * ZR while T <= 128
    const int Q = L >> 2, q0 = (l0 >> 2) - 1;
    float wf[FR], bf[FR], wz[ZR][2], bz[ZR];
    int zrow[ZR];
#pragma unroll
    for (int r = 0; r < FR; ++r) {
        const int o = wave * FR + r;
        wf[r] = a.lin_w[2][o * 64 + lane];
        bf[r] = a.lin_b[2][o];
    }
#pragma unroll
    for (int r = 0; r < ZR; ++r) {
        const int idx = wave * ZR + r, c = idx / s.n0, q = q0 + idx - c * s.n0;
        zrow[r] = (idx < 4 * s.n0 && q >= 0 && q < Q) ? c * Q + q : -1;
        const size_t row = zrow[r] >= 0 ? zrow[r] : 0;
        wz[r][0] = a.lin_w[3][row * 128 + lane];
        wz[r][1] = a.lin_w[3][row * 128 + lane + 64];
        bz[r] = a.lin_b[3][row];
    }
    cvae_stage_w(sm + s.w5, a.c_w[0], 32, 16 * 3, 32, tid);
    cvae_stage_w(sm + s.w6, a.c_w[1], F, 32 * 3, s.cbF, tid);
    cvae_stage_w(sm + s.w7, a.c_w[2], F, F * 3, s.cbF, tid);
    // post_y = py2(py0(y)); zy = [z | post_y]; fz_h = fz0(zy)
    float* py_h = sm + s.head;
    float* zy = py_h + 16;
    float* fz_h = zy + 64;
    if (tid < 32) zy[tid] = a.z[(size_t)n * 32 + tid];
    cvae_linear<2>(a.y + (size_t)n * 8, a.lin_w[0], a.lin_b[0], py_h, 8, 16, wave, lane);
    __syncthreads();
    cvae_linear<4>(py_h, a.lin_w[1], a.lin_b[1], zy + 32, 16, 32, wave, lane);
    __syncthreads();
    {   // fz_h = fz0(zy): In = 64, one product per lane, as small_linear_kernel sums it
        float t[FR];
#pragma unroll
        for (int r = 0; r < FR; ++r) {
            float v = 0.f;
            v += wf[r] * zy[lane];
            t[r] = wave_sum(v);
        }
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < FR; ++r) fz_h[wave * FR + r] = t[r] + bf[r];
        }
    }
    __syncthreads();
    {   // the slice of z0 = fz2(fz_h), viewed [4][L/4], that the tile reads: positions [l0/4 - 1, l0/4 - 1 + n0); zero outside [0, L/4)
        float* z0 = sm + s.z0;
        float t[ZR];
#pragma unroll
        for (int r = 0; r < ZR; ++r) {
            float v = 0.f;
            v += wz[r][0] * fz_h[lane];
            v += wz[r][1] * fz_h[lane + 64];
            t[r] = wave_sum(v);
        }
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < ZR; ++r)
                if (wave * ZR + r < 4 * s.n0) z0[wave * ZR + r] = zrow[r] >= 0 ? t[r] + bz[r] : 0.f;
        }
    }
    __syncthreads();
    cvae_convt_stage<2>(sm + s.z0, s.n0, a.t_w[0], a.t_b[0], a.t_s[0], a.t_t[0], sm + s.d1, s.n1, 4, 8, (l0 >> 1) - 2, L >> 1, wave, lane);
    __syncthreads();
    cvae_convt_stage<4>(sm + s.d1, s.n1, a.t_w[1], a.t_b[1], a.t_s[1], a.t_t[1], sm + s.d2, s.n2, 8, 16, l0 - 4, L, wave, lane);
    __syncthreads();
    cvae_conv_stage<false>(sm + s.d2, s.n2, 1, sm + s.w5, 32, a.c_b[0], a.c_s[0], a.c_t[0], sm + s.d3, s.n3, 16, 32, l0 - 2, L, wave, lane);
    __syncthreads();            // d2 and everything before it is dead: d4 overlays it
    cvae_conv_stage<false>(sm + s.d3, s.n3, 0, sm + s.w6, s.cbF, a.c_b[1], a.c_s[1], a.c_t[1], sm + s.d4, s.n4, 32, F, l0 - 1, L, wave, lane);
    __syncthreads();
    cvae_conv_stage<true>(sm + s.d4, s.n4, 0, sm + s.w7, s.cbF, a.c_b[2], nullptr, nullptr, a.out + (size_t)n * F * L, T, F, F, l0, L, wave, lane);
}

// out[row] = (a ? a[row] : 0) + b[(row / (rep*period)) * period + row % period]   (per-clip rows broadcast over `rep` draws)
__global__ __launch_bounds__(256) void add_bcast_kernel(const f4* __restrict__ a, const f4* __restrict__ b, f4* __restrict__ out,
                                                        size_t n4, int row_q, int period, int rep) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const size_t row = i / row_q;
        const size_t brow = (row / ((size_t)rep * period)) * period + row % period;
        const f4 bv = b[brow * row_q + (i - row * row_q)];
        out[i] = a ? a[i] + bv : bv;
    }
}

// out[(b * A + a) * inner + i] = in[(a * B + b) * inner + i]: swap the two leading axes of an [A, B, inner] array of 32-bit words
// (roll-out: utterance-major [U, W, ...] arguments <-> the window-major order phase A and the decoder steps work in)
template <typename V>
__global__ __launch_bounds__(256) void swap01_kernel(const V* __restrict__ in, V* __restrict__ out, int A, int B, size_t inner) {
    const size_t n = (size_t)A * B * inner;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t row = i / inner, c = i - row * inner;
        const size_t b = row / A, a = row - b * A;
        out[i] = in[(a * B + b) * inner + c];
    }
}

// Roll-out hand-off after window w (one launch per decoder step).  pose [U, F, D] is the step's raw output; prior_in [U, P, D] is the
// prior this step was seeded with (for w >= 1 the raw last P frames of window w-1); H = F - P.
//   track [U, T, D], T = W*H + P:  rows w*H + j = (1 - alpha[j]) * prior_in[j] + alpha[j] * pose[j] for j < P and w >= 1, pose[j] otherwise
//   windows [U, W, F, D] (optional): the raw pose;  prior_out [U, P, D]: pose[H + j], the next step's prior.
// alpha == nullptr: alpha[j] = (j + 1) / (P + 1).  prior_in and prior_out are different buffers (the caller ping-pongs), so no thread reads what another one writes.  The blend is
// two rounded products and one rounded sum (no fused multiply-add): the arithmetic a host restatement in fp32 reproduces bit for bit.
__global__ __launch_bounds__(256) void rollout_handoff_kernel(const float* __restrict__ pose, const float* __restrict__ prior_in,
                                                              const float* __restrict__ alpha, float* __restrict__ track,
                                                              float* __restrict__ windows, float* __restrict__ prior_out, int U, int W,
                                                              int w, int F, int P, int D) {
    const int H = F - P;
    const size_t T = (size_t)W * H + P, n = (size_t)U * F * D;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % D), j = (int)((i / D) % F), u = (int)(i / ((size_t)D * F));
        const float v = pose[i];
        float t = v;
        if (w > 0 && j < P) t = handoff_blend(alpha, j, P, prior_in[((size_t)u * P + j) * D + d], v);     // common.h: rounded products, rounded sum
        track[((size_t)u * T + (size_t)w * H + j) * D + d] = t;
        if (windows) windows[(((size_t)u * W + w) * F + j) * D + d] = v;
        if (j >= H) prior_out[((size_t)u * P + (j - H)) * D + d] = v;
    }
}

// out[(u * W + w), i] = audio[u, w * hop + i]: the overlapping windows of a long recording as a batch of clips.  A window that runs past
// the end of the track holds L = total - w * hop < n samples and is completed as make_audio_fixed_length does (np.pad mode="symmetric":
// the samples mirrored about the end, the last one repeated, with period 2L).
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ audio, float* __restrict__ out, int U, int64_t total,
                                                            int W, int64_t hop, int n) {
    const size_t cnt = (size_t)U * W * n;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (size_t)gridDim.x * 256) {
        const size_t clip = i / n;
        const int64_t start = (int64_t)(clip % W) * hop, L = total - start;     // L >= 1 (checked by the launcher)
        int64_t k = (int64_t)(i - clip * n);
        if (k >= L) {
            k %= 2 * L;
            if (k >= L) k = 2 * L - 1 - k;
        }
        out[i] = audio[(clip / W) * (size_t)total + start + k];
    }
}

inline int grid_for(size_t n, int cap = 4096) {
    const size_t g = (n + 255) / 256;
    return (int)(g < (size_t)cap ? (g ? g : 1) : cap);
}

}  // namespace

// ================================ C ABI + internal launchers =============================================

int egi_layernorm(const float* x, const float* gamma, const float* beta, float* y, void* img, int rows, int d, float eps, hipStream_t st) {
    EG_REQUIRE(x && gamma && beta && y && rows > 0, EG_ERR_BAD_ARG, "eg_layernorm: null pointer");
    EG_REQUIRE(d > 0 && d <= 2048, EG_ERR_UNSUPPORTED, "eg_layernorm: D=%d", d);
    EG_REQUIRE(!img || (d & 63) == 0, EG_ERR_ALIGN, "layernorm image output needs D %% 64 == 0");
    unsigned short* im = reinterpret_cast<unsigned short*>(img);
    dim3 grid(eg_cdiv(rows, 4)), block(256);
    if (d & 3) {
        hipLaunchKernelGGL(layernorm_any_kernel, grid, block, 0, st, x, gamma, beta, y, rows, d, eps);
        return eg_check_launch("layernorm");
    }
    if (d <= 256) hipLaunchKernelGGL((layernorm_kernel<1>), grid, block, 0, st, x, gamma, beta, y, rows, d, eps, im);
    else if (d <= 512) hipLaunchKernelGGL((layernorm_kernel<2>), grid, block, 0, st, x, gamma, beta, y, rows, d, eps, im);
    else if (d <= 1024) hipLaunchKernelGGL((layernorm_kernel<4>), grid, block, 0, st, x, gamma, beta, y, rows, d, eps, im);
    else hipLaunchKernelGGL((layernorm_kernel<8>), grid, block, 0, st, x, gamma, beta, y, rows, d, eps, im);
    return eg_check_launch("layernorm");
}
extern "C" int eg_layernorm_img(const float* x, const float* gamma, const float* beta, float* y, void* y_images, int32_t rows, int32_t d, float eps,
                                void* stream) {
    return egi_layernorm(x, gamma, beta, y, y_images, rows, d, eps, (hipStream_t)stream);
}
extern "C" int eg_layernorm(const float* x, const float* gamma, const float* beta, float* y, int32_t rows, int32_t d,
                            float eps, void* stream) {
    return egi_layernorm(x, gamma, beta, y, nullptr, rows, d, eps, (hipStream_t)stream);
}


extern "C" int eg_reparameterize(const float* mu, const float* logvar, const float* eps, float* z, int64_t n, void* stream) {
    EG_REQUIRE(mu && logvar && eps && z && n > 0, EG_ERR_BAD_ARG, "eg_reparameterize: null pointer");
    hipLaunchKernelGGL(reparam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mu, logvar, eps, z, n);
    return eg_check_launch("reparameterize");
}

extern "C" int eg_add_rows(const float* a, const float* table, float* out, int64_t rows, int32_t d, int32_t period, void* stream) {
    EG_REQUIRE(a && table && out && rows > 0 && d > 0, EG_ERR_BAD_ARG, "eg_add_rows: null pointer or empty shape");
    if (d & 3) {
        const size_t n = (size_t)rows * d;
        hipLaunchKernelGGL(add_rows_any_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, a, table, out, n, d, period);
        return eg_check_launch("add_rows");
    }
    const size_t n4 = (size_t)rows * (d / 4);
    hipLaunchKernelGGL(add_kernel, dim3(grid_for(n4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const f4*>(a),
                       reinterpret_cast<const f4*>(table), reinterpret_cast<f4*>(out), n4, d / 4, period);
    return eg_check_launch("add_rows");
}

int egi_add_img(const float* a, const float* b, float* out, void* img, size_t n, int row_len, int period, hipStream_t st);
// eg_add_rows with a second output: the sum as bf16 (hi, lo) tile-planar images (eg_split_tiles layout of width d) for a pre-split product
extern "C" int eg_add_rows_split(const float* a, const float* table, float* out, void* images, int64_t rows, int32_t d, int32_t period, void* stream) {
    EG_REQUIRE(a && table && out && images && rows > 0 && d > 0 && (d & 63) == 0, EG_ERR_BAD_ARG, "eg_add_rows_split: null pointer, empty shape or d %% 64 != 0");
    return egi_add_img(a, table, out, images, (size_t)rows * d, d, period, (hipStream_t)stream);
}

extern "C" int eg_window_gather(const float* audio, int32_t utterances, int64_t total_samples, int32_t windows, int64_t hop_samples,
                                int32_t n_samples, float* out, void* stream) {
    EG_REQUIRE(audio && out, EG_ERR_BAD_ARG, "eg_window_gather: null pointer");
    EG_REQUIRE(utterances >= 1 && windows >= 1, EG_ERR_BAD_ARG, "eg_window_gather: utterances=%d windows=%d", utterances, windows);
    EG_REQUIRE(total_samples >= 1 && hop_samples >= 1 && n_samples >= 1, EG_ERR_BAD_ARG, "eg_window_gather: total_samples=%lld hop_samples=%lld n_samples=%d",
               (long long)total_samples, (long long)hop_samples, n_samples);
    EG_REQUIRE((int64_t)(windows - 1) * hop_samples < total_samples, EG_ERR_BAD_ARG,
               "eg_window_gather: windows=%d: the last window starts at sample %lld of %lld", windows, (long long)(windows - 1) * hop_samples,
               (long long)total_samples);
    hipLaunchKernelGGL(window_gather_kernel, dim3(grid_for((size_t)utterances * windows * n_samples)), dim3(256), 0, (hipStream_t)stream, audio, out,
                       utterances, total_samples, windows, hop_samples, n_samples);
    return eg_check_launch("window_gather");
}

// ---- internal (C++ linkage) launchers used by generator.hip ------------------------------------------------
int egi_embedding(const int64_t* idx, const float* table, float* out, int rows, int dim, int ld, int n_words, hipStream_t st) {
    hipLaunchKernelGGL(embedding_kernel, dim3(grid_for((size_t)rows * dim / 4)), dim3(256), 0, st, idx, table, out, rows, dim, ld, n_words);
    return eg_check_launch("embedding");
}
int egi_add(const float* a, const float* b, float* out, size_t n, int row_len, int period, hipStream_t st);
int egi_embedding_img(const int64_t* idx, const float* table, float* out, void* img, void* zero_line, int rows, int dim, int ld, int n_words, hipStream_t st) {
    EG_REQUIRE((dim & 3) == 0 && (ld & 63) == 0 && ld >= dim, EG_ERR_ALIGN, "embedding: dim %% 4, ld %% 64");
    bf8* hi = reinterpret_cast<bf8*>(img);
    bf8* lo = hi + (size_t)eg_cdiv(rows, 64) * (ld >> 3) * 64;
    hipLaunchKernelGGL(embedding_img_kernel, dim3(grid_for((size_t)eg_cdiv(rows, 64) * 64 * (ld >> 3))), dim3(256), 0, st, idx, table, out, hi, lo,
                       reinterpret_cast<bf8*>(zero_line), rows, dim, ld, n_words);
    return eg_check_launch("embedding");
}
// img != nullptr: also the sum's bf16 (hi, lo) images of width row_len (row_len % 64 == 0), hi then lo image
int egi_add_img(const float* a, const float* b, float* out, void* img, size_t n, int row_len, int period, hipStream_t st) {
    if (!img) return egi_add(a, b, out, n, row_len, period, st);
    EG_REQUIRE((row_len & 63) == 0, EG_ERR_ALIGN, "add: image output needs row_len %% 64 == 0");
    const size_t rows = n / row_len;
    bf8* hi = reinterpret_cast<bf8*>(img);
    bf8* lo = hi + ((rows + 63) >> 6) * (size_t)(row_len >> 3) * 64;
    hipLaunchKernelGGL(add_img_kernel, dim3(grid_for(n / 8)), dim3(256), 0, st, reinterpret_cast<const f4*>(a), reinterpret_cast<const f4*>(b),
                       reinterpret_cast<f4*>(out), hi, lo, rows, row_len / 8, period);
    return eg_check_launch("add");
}
int egi_add(const float* a, const float* b, float* out, size_t n, int row_len, int period, hipStream_t st) {
    hipLaunchKernelGGL(add_kernel, dim3(grid_for(n / 4)), dim3(256), 0, st, reinterpret_cast<const f4*>(a),
                       reinterpret_cast<const f4*>(b), reinterpret_cast<f4*>(out), n / 4, row_len / 4, period);
    return eg_check_launch("add");
}
int egi_add_bcast(const float* a, const float* b, float* out, size_t rows, int row_len, int period, int rep, hipStream_t st) {
    const size_t n4 = rows * (size_t)(row_len / 4);
    hipLaunchKernelGGL(add_bcast_kernel, dim3(grid_for(n4)), dim3(256), 0, st, reinterpret_cast<const f4*>(a),
                       reinterpret_cast<const f4*>(b), reinterpret_cast<f4*>(out), n4, row_len / 4, period, rep);
    return eg_check_launch("add_bcast");
}
// EG_TIME_LINEAR (read per call, like EG_GEMM_TILE): unset or empty = the register-blocked kernel; "ref" = the reference form (A/B runs and the
// bit-equality check of tests/test_gpu_time_linear_blocked.py, this round only).  Anything else is refused before any launch.
int egi_time_linear(const float* x, const float* w, const float* bias, float* y, int batch, int L, int C, int ld, hipStream_t st) {
    const char* e = getenv("EG_TIME_LINEAR");
    const bool ref = e && !strcmp(e, "ref");
    EG_REQUIRE(!e || !e[0] || ref, EG_ERR_BAD_ARG, "EG_TIME_LINEAR=\"%s\": the only accepted value is \"ref\" (unset or empty: register-blocked)", e);
    const size_t smem = sizeof(float) * ((size_t)L * (ref ? L : (L + 3) & ~3) + (size_t)L * 64);
    EG_REQUIRE(smem <= 65536, EG_ERR_UNSUPPORTED, "time_linear: L=%d needs %zu bytes of LDS", L, smem);
    if (ref)
        hipLaunchKernelGGL(time_linear_ref_kernel, dim3(eg_cdiv(C, 64), batch), dim3(256), smem, st, x, w, bias, y, L, C, ld);
    else
        hipLaunchKernelGGL(time_linear_kernel, dim3(eg_cdiv(C, 64), batch), dim3(256), smem, st, x, w, bias, y, L, C, ld);
    return eg_check_launch("time_linear");
}
// TextEncoderTCN.fc1 on its own (the generator calls egi_time_linear directly)
extern "C" int eg_time_linear(const float* x, const float* w, const float* bias, float* y, int32_t batch, int32_t len, int32_t c, int32_t ld,
                              void* stream) {
    EG_REQUIRE(x && w && bias && y, EG_ERR_BAD_ARG, "eg_time_linear: null pointer");
    EG_REQUIRE(batch > 0 && len > 0 && c > 0 && ld >= c, EG_ERR_BAD_ARG, "eg_time_linear: batch=%d len=%d c=%d ld=%d", batch, len, c, ld);
    return egi_time_linear(x, w, bias, y, batch, len, c, ld, (hipStream_t)stream);
}
int egi_copy2d(const float* src, int lds_, float* dst, int ldd, int rows, int cols, hipStream_t st) {
    hipLaunchKernelGGL(copy2d_kernel, dim3(grid_for((size_t)rows * cols)), dim3(256), 0, st, src, lds_, dst, ldd, rows, cols);
    return eg_check_launch("copy2d");
}

int egi_swap01(const void* in, void* out, int A, int B, size_t inner_words, hipStream_t st) {
    if ((inner_words & 3) == 0 && eg_aligned16(in) && eg_aligned16(out)) {
        const size_t q = inner_words / 4;
        hipLaunchKernelGGL((swap01_kernel<u32x4_t>), dim3(grid_for((size_t)A * B * q)), dim3(256), 0, st, reinterpret_cast<const u32x4_t*>(in),
                           reinterpret_cast<u32x4_t*>(out), A, B, q);
    } else {
        hipLaunchKernelGGL((swap01_kernel<unsigned int>), dim3(grid_for((size_t)A * B * inner_words)), dim3(256), 0, st,
                           reinterpret_cast<const unsigned int*>(in), reinterpret_cast<unsigned int*>(out), A, B, inner_words);
    }
    return eg_check_launch("swap01");
}
int egi_rollout_handoff(const float* pose, const float* prior_in, const float* alpha, float* track, float* windows, float* prior_out, int U,
                        int W, int w, int F, int P, int D, hipStream_t st) {
    hipLaunchKernelGGL(rollout_handoff_kernel, dim3(grid_for((size_t)U * F * D)), dim3(256), 0, st, pose, prior_in, alpha, track, windows,
                       prior_out, U, W, w, F, P, D);
    return eg_check_launch("rollout_handoff");
}

struct EgiPriorW {
    const float *w1, *b1, *s1, *t1, *w2, *b2, *s2, *t2;
    const float *sp_w0, *sp_b0, *sp_w1, *sp_b1, *tc_w0, *tc_b0, *tc_w1, *tc_b1, *tm_w0, *tm_b0, *tm_w1, *tm_b1;
};
int egi_prior_encoder(const float* prior, const EgiPriorW& w, float* cat, float* tm_mem, float* tm_pe, float* tm_gram,
                      int batch, int P, int F, int D, int Dpad, int chunk, int variant, hipStream_t st) {
    PriorArgs a;
    a.prior = prior; a.w1 = w.w1; a.b1 = w.b1; a.s1 = w.s1; a.t1 = w.t1; a.w2 = w.w2; a.b2 = w.b2; a.s2 = w.s2; a.t2 = w.t2;
    a.sp_w0 = w.sp_w0; a.sp_b0 = w.sp_b0; a.sp_w1 = w.sp_w1; a.sp_b1 = w.sp_b1;
    a.tc_w0 = w.tc_w0; a.tc_b0 = w.tc_b0; a.tc_w1 = w.tc_w1; a.tc_b1 = w.tc_b1;
    a.tm_w0 = w.tm_w0; a.tm_b0 = w.tm_b0; a.tm_w1 = w.tm_w1; a.tm_b1 = w.tm_b1;
    a.cat = cat; a.tm_mem = tm_mem; a.tm_pe = tm_pe;
    a.P = P; a.PL = F - P; a.D = D; a.Dpad = Dpad; a.chunk = chunk; a.variant = variant;
    const int PL = F - P;
    a.dchunk = variant == 1 ? D : (D < 64 ? D : 64);
    const int dc = a.dchunk;
    const size_t base = sizeof(float) * ((size_t)P * (dc + 4) + (size_t)PL * (dc + 2) + (size_t)PL * dc +
                                         (variant == 1 ? (size_t)chunk * D + 2 * (size_t)D : 0));
    const size_t wbytes = sizeof(float) * ((size_t)PL * P * 3 + (size_t)PL * PL * 3);
    a.stage_w = (base + wbytes <= 160 * 1024) ? 1 : 0;          // conv weights in LDS when they fit, else read through L1
    const size_t smem = base + (a.stage_w ? wbytes : 0);
    if (smem > 160 * 1024) { eg_set_error("prior encoder: LDS need %zu B", smem); return EG_ERR_UNSUPPORTED; }
    if (int rc = eg_ensure_dynamic_lds(reinterpret_cast<const void*>(prior_pred_kernel), smem, "prior encoder")) return rc;
    hipLaunchKernelGGL(prior_pred_kernel, dim3(batch, eg_cdiv(D, dc)), dim3(256), smem, st, a);
    int rc = eg_check_launch("prior_pred");
    if (rc || variant != 1) return rc;
    hipLaunchKernelGGL(tm_gram_kernel, dim3(eg_cdiv(D * chunk, 256)), dim3(256), 0, st, tm_mem, tm_pe, tm_gram, batch, D, chunk);
    if ((rc = eg_check_launch("tm_gram"))) return rc;
    hipLaunchKernelGGL(tm_apply_kernel, dim3(batch), dim3(64), 0, st, tm_mem, tm_gram, cat, D, Dpad, chunk, P, F);
    return eg_check_launch("tm_apply");
}

int egi_conv1d(const float* x, const float* w, const float* bias, const float* scale, const float* shift, float* y, int n, int cin,
               int cout, int lin, int k, int stride, int pad, int act, hipStream_t st) {
    const int lout = (lin + 2 * pad - k) / stride + 1;
    const int per_wave = eg_cdiv(cout, 4);
    const int cog = per_wave <= 4 ? 4 : (per_wave <= 8 ? 8 : 16);
    const size_t smem = sizeof(float) * ((((size_t)cin * (63 * stride + k) + 3) & ~(size_t)3) + (size_t)cin * k * 4 * cog);
    if (smem > 160 * 1024) { eg_set_error("conv1d: LDS need %zu B", smem); return EG_ERR_UNSUPPORTED; }
    {
        const void* kp = cog == 4 ? reinterpret_cast<const void*>(conv1d_kernel<4>)
                                  : (cog == 8 ? reinterpret_cast<const void*>(conv1d_kernel<8>) : reinterpret_cast<const void*>(conv1d_kernel<16>));
        if (int rc = eg_ensure_dynamic_lds(kp, smem, "conv1d")) return rc;
    }
    dim3 grid(eg_cdiv(lout, 64), n, eg_cdiv(cout, 4 * cog));
    if (cog == 4)
        hipLaunchKernelGGL((conv1d_kernel<4>), grid, dim3(256), smem, st, x, w, bias, scale, shift, y, cin, cout, lin, lout, k, stride, pad, act);
    else if (cog == 8)
        hipLaunchKernelGGL((conv1d_kernel<8>), grid, dim3(256), smem, st, x, w, bias, scale, shift, y, cin, cout, lin, lout, k, stride, pad, act);
    else
        hipLaunchKernelGGL((conv1d_kernel<16>), grid, dim3(256), smem, st, x, w, bias, scale, shift, y, cin, cout, lin, lout, k, stride, pad, act);
    return eg_check_launch("conv1d");
}
extern "C" int eg_conv1d(const float* x, const float* w, const float* bias, const float* scale, const float* shift, float* y, int32_t n,
                         int32_t cin, int32_t cout, int32_t lin, int32_t k, int32_t stride, int32_t pad, int32_t act, void* stream) {
    EG_REQUIRE(x && w && bias && y && n > 0 && cin > 0 && cout > 0 && lin > 0, EG_ERR_BAD_ARG, "eg_conv1d: null pointer or empty shape");
    EG_REQUIRE(k >= 1 && stride >= 1 && pad >= 0 && lin + 2 * pad >= k, EG_ERR_BAD_ARG, "eg_conv1d: k=%d stride=%d pad=%d lin=%d", k, stride, pad, lin);
    EG_REQUIRE((scale == nullptr) == (shift == nullptr), EG_ERR_BAD_ARG, "eg_conv1d: scale and shift come together");
    return egi_conv1d(x, w, bias, scale, shift, y, n, cin, cout, lin, k, stride, pad, act, (hipStream_t)stream);
}
int egi_convt1d(const float* x, const float* w, const float* bias, const float* scale, const float* shift, float* y, int n, int cin,
                int cout, int lin, hipStream_t st) {
    hipLaunchKernelGGL(convt1d_kernel, dim3(eg_cdiv(2 * lin, 128), n), dim3(128), 0, st, x, w, bias, scale, shift, y, cin, cout, lin);
    return eg_check_launch("convt1d");
}
int egi_small_linear(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int n, int in, int out,
                     hipStream_t st) {
    hipLaunchKernelGGL(small_linear_kernel, dim3(eg_cdiv(out, 4) < 64 ? eg_cdiv(out, 4) : 64, n), dim3(256), 0, st, x, ldx, w, bias, y,
                       ldy, in, out);
    return eg_check_launch("small_linear");
}
// The whole of eg_cvae_sample in one launch.  *taken = 0 (and nothing launched) where the staged weights and the tile do not fit the LDS
// (frames = 120: the last stage's weights alone are 172 KB): the caller then runs the launch chain.  The tile of the d_model axis is
// 128 positions (64 and 256 were measured slower), the whole axis where that is shorter.
int egi_cvae_sample_fused(EgiCvaeFused a, int n, hipStream_t st, int* taken) {
    *taken = 0;
    const int T = a.L < 128 ? a.L : 128;
    if (a.L % 4 != 0 || n > 65535) return EG_OK;
    const size_t smem = sizeof(float) * (size_t)cvae_fused_lds(a.F, T).total;
    if (smem > 160 * 1024) return EG_OK;
    if (int rc = eg_ensure_dynamic_lds(reinterpret_cast<const void*>(cvae_sample_fused_kernel), smem, "cvae sample")) return rc;
    a.T = T;
    hipLaunchKernelGGL(cvae_sample_fused_kernel, dim3(eg_cdiv(a.L, T), n), dim3(64 * CVAE_WAVES), smem, st, a);
    *taken = 1;
    return eg_check_launch("cvae_sample_fused");
}


// ---- SoftmaxContrastiveLoss (test_emotion_gesture_diversity_iterative.py:80-127) -------------------------------------------
namespace {
// one workgroup per face row i: cross[i][:] (each thread owns columns j = tid, tid+256, ...), then the row's logsumexp / argmax
__global__ __launch_bounds__(256) void contrastive_rows_kernel(const float* __restrict__ face, const float* __restrict__ audio, int n, int d,
                                                               float* __restrict__ cross, float* __restrict__ row_loss,
                                                               int* __restrict__ row_hit) {
    extern __shared__ float sh[];                 // d normalised face values, then 256 x (max, argmax) / sums
    float* f = sh;
    float* red = sh + d;
    int* redi = reinterpret_cast<int*>(red + 256);
    const int i = blockIdx.x, tid = threadIdx.x;
    float part = 0.f;
    for (int k = tid; k < d; k += 256) { const float v = face[(size_t)i * d + k]; f[k] = v; part += v * v; }
    red[tid] = part;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    const float finv = 1.f / fmaxf(sqrtf(red[0]), 1e-12f);
    __syncthreads();
    float vmax = -INFINITY, diag = 0.f;
    int amax = 0x7fffffff;
    float* crow = cross ? cross + (size_t)i * n : nullptr;
    // pass 1: values, row maximum and its first index
    for (int j = tid; j < n; j += 256) {
        const float* a = audio + (size_t)j * d;
        float na = 0.f;
        for (int k = 0; k < d; ++k) na += a[k] * a[k];
        const float ainv = 1.f / fmaxf(sqrtf(na), 1e-12f);
        float dist = 0.f;
        for (int k = 0; k < d; ++k) { const float t = f[k] * finv - a[k] * ainv; dist += t * t; }
        const float c = fmaxf(1.f / (sqrtf(dist) + 1e-8f), 1e-8f);
        if (crow) crow[j] = c;
        if (j == i) diag = c;
        if (c > vmax) { vmax = c; amax = j; }
    }
    red[tid] = vmax; redi[tid] = amax;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const float o = red[tid + s]; const int oi = redi[tid + s];
            if (o > red[tid] || (o == red[tid] && oi < redi[tid])) { red[tid] = o; redi[tid] = oi; }
        }
        __syncthreads();
    }
    const float m = red[0];
    const int am = redi[0];
    __syncthreads();
    // pass 2: sum exp(c - m); recompute c (cross may be absent) exactly as above
    float se = 0.f;
    for (int j = tid; j < n; j += 256) {
        const float* a = audio + (size_t)j * d;
        float na = 0.f;
        for (int k = 0; k < d; ++k) na += a[k] * a[k];
        const float ainv = 1.f / fmaxf(sqrtf(na), 1e-12f);
        float dist = 0.f;
        for (int k = 0; k < d; ++k) { const float t = f[k] * finv - a[k] * ainv; dist += t * t; }
        const float c = fmaxf(1.f / (sqrtf(dist) + 1e-8f), 1e-8f);
        se += expf(c - m);
    }
    red[tid] = se;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    // the diagonal value lives in exactly one thread
    __shared__ float sdiag;
    if (i % 256 == tid) sdiag = diag;
    __syncthreads();
    if (tid == 0) {
        row_loss[i] = m + logf(red[0]) - sdiag;
        row_hit[i] = (am == i) ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void contrastive_mean_kernel(const float* __restrict__ row_loss, const int* __restrict__ row_hit, int n,
                                                               float* __restrict__ loss, float* __restrict__ acc) {
    __shared__ float rl[256];
    __shared__ int rh[256];
    const int tid = threadIdx.x;
    float l = 0.f; int h = 0;
    for (int i = tid; i < n; i += 256) { l += row_loss[i]; h += row_hit[i]; }
    rl[tid] = l; rh[tid] = h;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) { rl[tid] += rl[tid + s]; rh[tid] += rh[tid + s]; } __syncthreads(); }
    if (tid == 0) { *loss = rl[0] / (float)n; *acc = (float)rh[0] / (float)n; }
}
// ---- backward of the loss above --------------------------------------------------------------------------------------------
// L = mean_i (logsumexp_j c_ij - c_ii), c_ij = max(1 / (D_ij + 1e-8), 1e-8), D_ij = || fh_i - ah_j ||, fh = f / max(||f||, 1e-12) (F.normalize).
//   G_ij = (softmax_j(c_i.) - [i == j]) / n;   dc/dD = -c^2 (0 where the clamp is active);   dD/dfh_i = (fh_i - ah_j) / D (0 at D = 0, as torch.norm)
//   W_ij = -G_ij c_ij^2 / D_ij;   g_fh_i = sum_j W_ij (fh_i - ah_j);   g_ah_j = -sum_i W_ij (fh_i - ah_j) (both summed term by term);   g_x = (g_xh - xh (xh . g_xh)) / ||x||
// Three launches: the 2n inverse norms; one workgroup per row i (softmax of its row, W row, face gradient); one per column j (audio gradient).
__global__ __launch_bounds__(256) void contrastive_norms_kernel(const float* __restrict__ face, const float* __restrict__ audio, int n, int d,
                                                                float* __restrict__ inv) {
    __shared__ float red[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* x = (r < n ? face + (size_t)r * d : audio + (size_t)(r - n) * d);
    float part = 0.f;
    for (int k = tid; k < d; k += 256) part += x[k] * x[k];
    red[tid] = part;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    if (tid == 0) inv[r] = 1.f / fmaxf(sqrtf(red[0]), 1e-12f);
}
__device__ __forceinline__ float block_sum256(float v, float* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    return red[0];
}
__device__ __forceinline__ float block_max256(float v, float* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]); __syncthreads(); }
    return red[0];
}
// || fh - a ainv ||^2 in four interleaved chains (k % 4) combined pairwise -- the same value wherever the backward needs a distance.  One chain
// of d squares drifts enough at d = 257 to take the gradients to ~0.7 of the tolerance of their float64 test; four chains stay under half.
__device__ __forceinline__ float dist2_four(const float* __restrict__ fh, const float* __restrict__ a, float ainv, int d) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int k = 0;
    for (; k + 3 < d; k += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) { const float t = fh[k + u] - a[k + u] * ainv; s[u] += t * t; }
    }
#pragma unroll
    for (int u = 0; u < 3; ++u)
        if (k + u < d) { const float t = fh[k + u] - a[k + u] * ainv; s[u] += t * t; }
    return (s[0] + s[1]) + (s[2] + s[3]);
}
__global__ __launch_bounds__(256) void contrastive_bwd_rows_kernel(const float* __restrict__ face, const float* __restrict__ audio,
                                                                   const float* __restrict__ inv, int n, int d, float* __restrict__ Wm,
                                                                   float* __restrict__ gface) {
    extern __shared__ float sh[];                 // fh_i [d], then 256 reduction slots
    float* f = sh;
    float* red = sh + d;
    const int i = blockIdx.x, tid = threadIdx.x;
    const float finv = inv[i];
    for (int k = tid; k < d; k += 256) f[k] = face[(size_t)i * d + k] * finv;
    __syncthreads();
    float* wrow = Wm + (size_t)i * n;
    // pass 1: c_ij -> wrow, D_ij is recomputed in pass 3 from c (D = 1/c - 1e-8 would lose bits: recompute the distance instead)
    float vmax = -INFINITY;
    for (int j = tid; j < n; j += 256) {
        const float* a = audio + (size_t)j * d;
        const float ainv = inv[n + j];
        const float dist = dist2_four(f, a, ainv, d);
        const float c = fmaxf(1.f / (sqrtf(dist) + 1e-8f), 1e-8f);
        wrow[j] = c;
        vmax = fmaxf(vmax, c);
    }
    const float m = block_max256(vmax, red);
    float se = 0.f;
    for (int j = tid; j < n; j += 256) se += expf(wrow[j] - m);
    const float denom = block_sum256(se, red);
    // pass 3: W_ij
    for (int j = tid; j < n; j += 256) {
        const float* a = audio + (size_t)j * d;
        const float ainv = inv[n + j];
        const float dist = dist2_four(f, a, ainv, d);
        const float D = sqrtf(dist), c = wrow[j];
        const float G = (expf(c - m) / denom - (j == i ? 1.f : 0.f)) / (float)n;
        const bool live = D > 0.f && (1.f / (D + 1e-8f)) > 1e-8f;
        const float w = live ? -G * c * c / D : 0.f;
        wrow[j] = w;
    }
    __syncthreads();                                // orders the wrow writes before the reads below
    // g_fh[k] = sum_j W_ij (fh[k] - ah_j[k]), term by term: the factored form fh[k] sum_j W_ij - sum_j W_ij ah_j[k] subtracts two sums of size
    // |W| where the terms are of size |W| D, and loses a factor 1 / D for a face row that lies next to an audio row.  Then through the normalisation.
    float dotp = 0.f;
    for (int k = tid; k < d; k += 256) {
        // four interleaved chains (j % 4), then pairwise: one chain of n terms alone puts the gradient at ~1x the tolerance its float64 test allows
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        int j = 0;
        for (; j + 3 < n; j += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] += wrow[j + u] * (f[k] - audio[(size_t)(j + u) * d + k] * inv[n + j + u]);
        }
#pragma unroll
        for (int u = 0; u < 3; ++u)
            if (j + u < n) acc[u] += wrow[j + u] * (f[k] - audio[(size_t)(j + u) * d + k] * inv[n + j + u]);
        const float g = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        gface[(size_t)i * d + k] = g;               // g_fh for now
        dotp += f[k] * g;
    }
    const float dot = block_sum256(dotp, red);
    for (int k = tid; k < d; k += 256) gface[(size_t)i * d + k] = (gface[(size_t)i * d + k] - f[k] * dot) * finv;
}
__global__ __launch_bounds__(256) void contrastive_bwd_cols_kernel(const float* __restrict__ face, const float* __restrict__ audio,
                                                                   const float* __restrict__ inv, const float* __restrict__ Wm, int n, int d,
                                                                   float* __restrict__ gaudio) {
    extern __shared__ float sh[];
    float* ah = sh;
    float* red = sh + d;
    const int j = blockIdx.x, tid = threadIdx.x;
    const float ainv = inv[n + j];
    for (int k = tid; k < d; k += 256) ah[k] = audio[(size_t)j * d + k] * ainv;
    __syncthreads();
    float dotp = 0.f;
    for (int k = tid; k < d; k += 256) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};        // -sum_i W_ij (fh_i[k] - ah_j[k]), term by term in four chains as in the row kernel
        int i = 0;
        for (; i + 3 < n; i += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] += Wm[(size_t)(i + u) * n + j] * (ah[k] - face[(size_t)(i + u) * d + k] * inv[i + u]);
        }
#pragma unroll
        for (int u = 0; u < 3; ++u)
            if (i + u < n) acc[u] += Wm[(size_t)(i + u) * n + j] * (ah[k] - face[(size_t)(i + u) * d + k] * inv[i + u]);
        const float g = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        gaudio[(size_t)j * d + k] = g;
        dotp += ah[k] * g;
    }
    const float dot = block_sum256(dotp, red);
    for (int k = tid; k < d; k += 256) gaudio[(size_t)j * d + k] = (gaudio[(size_t)j * d + k] - ah[k] * dot) * ainv;
}
}  // namespace

extern "C" int64_t eg_contrastive_backward_workspace_bytes(int32_t n) { return n > 0 ? ((int64_t)n * n + 2 * (int64_t)n) * 4 : 0; }
// d loss / d face, d loss / d audio for an upstream gradient of 1 (scale afterwards).
extern "C" int eg_contrastive_loss_backward(const float* face, const float* audio, int32_t n, int32_t d, float* gface, float* gaudio, void* workspace,
                                            int64_t workspace_bytes, void* stream) {
    EG_REQUIRE(face && audio && gface && gaudio && workspace, EG_ERR_BAD_ARG, "eg_contrastive_loss_backward: null pointer");
    EG_REQUIRE(n >= 1 && n <= 4096 && d >= 1 && d <= 8192, EG_ERR_BAD_ARG, "eg_contrastive_loss_backward: n=%d d=%d out of range", n, d);
    EG_REQUIRE(workspace_bytes >= eg_contrastive_backward_workspace_bytes(n), EG_ERR_WORKSPACE, "eg_contrastive_loss_backward: workspace %lld < %lld",
               (long long)workspace_bytes, (long long)eg_contrastive_backward_workspace_bytes(n));
    float* Wm = static_cast<float*>(workspace);
    float* inv = Wm + (size_t)n * n;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)(d + 256) * sizeof(float);
    hipLaunchKernelGGL(contrastive_norms_kernel, dim3(2 * n), dim3(256), 0, st, face, audio, n, d, inv);
    if (int rc = eg_check_launch("contrastive_norms")) return rc;
    hipLaunchKernelGGL(contrastive_bwd_rows_kernel, dim3(n), dim3(256), lds, st, face, audio, inv, n, d, Wm, gface);
    if (int rc = eg_check_launch("contrastive_bwd_rows")) return rc;
    hipLaunchKernelGGL(contrastive_bwd_cols_kernel, dim3(n), dim3(256), lds, st, face, audio, inv, Wm, n, d, gaudio);
    return eg_check_launch("contrastive_bwd_cols");
}

extern "C" int64_t eg_contrastive_workspace_bytes(int32_t n) { return n > 0 ? (int64_t)n * 8 : 0; }

extern "C" int eg_contrastive_loss(const float* face, const float* audio, int32_t n, int32_t d, float* cross, float* loss, float* acc,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    EG_REQUIRE(face && audio && loss && acc && workspace, EG_ERR_BAD_ARG, "eg_contrastive_loss: null pointer");
    EG_REQUIRE(n >= 1 && n <= 4096 && d >= 1 && d <= 8192, EG_ERR_BAD_ARG, "eg_contrastive_loss: n=%d d=%d out of range", n, d);
    EG_REQUIRE(workspace_bytes >= eg_contrastive_workspace_bytes(n), EG_ERR_WORKSPACE, "eg_contrastive_loss: workspace %lld < %lld",
               (long long)workspace_bytes, (long long)eg_contrastive_workspace_bytes(n));
    float* row_loss = static_cast<float*>(workspace);
    int* row_hit = reinterpret_cast<int*>(row_loss + n);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)(d + 512) * sizeof(float);
    hipLaunchKernelGGL(contrastive_rows_kernel, dim3(n), dim3(256), lds, st, face, audio, n, d, cross, row_loss, row_hit);
    int rc = eg_check_launch("contrastive_rows");
    if (rc != EG_OK) return rc;
    hipLaunchKernelGGL(contrastive_mean_kernel, dim3(1), dim3(256), 0, st, row_loss, row_hit, n, loss, acc);
    return eg_check_launch("contrastive_mean");
}

// ---- kernels the generator and the CVAE launch internally, on their own (tests compare each with float64; contracts in include/emogest.h) ----
extern "C" int eg_prior_encoder(const float* prior, const float* const* conv, const float* const* mem, float* cat, float* tm_mem, float* tm_pe,
                                float* tm_gram, int32_t batch, int32_t prior_frames, int32_t frames, int32_t d, int32_t dpad, int32_t chunk,
                                int32_t variant, void* stream) {
    EG_REQUIRE(prior && conv && cat, EG_ERR_BAD_ARG, "eg_prior_encoder: null pointer");
    EG_REQUIRE(variant == 0 || variant == 1, EG_ERR_BAD_ARG, "eg_prior_encoder: variant=%d", variant);
    EG_REQUIRE(batch > 0 && prior_frames > 0 && frames > prior_frames && d > 0, EG_ERR_BAD_ARG, "eg_prior_encoder: batch=%d prior_frames=%d frames=%d d=%d",
               batch, prior_frames, frames, d);
    EG_REQUIRE(dpad >= d, EG_ERR_BAD_ARG, "eg_prior_encoder: dpad=%d < d=%d", dpad, d);
    for (int i = 0; i < 8; ++i) EG_REQUIRE(conv[i], EG_ERR_BAD_ARG, "eg_prior_encoder: conv[%d] is null", i);
    int set = 0;
    for (int i = 0; mem && i < 12; ++i) set += mem[i] ? 1 : 0;
    EG_REQUIRE(set == 0 || set == 12, EG_ERR_BAD_ARG, "eg_prior_encoder: memory pointers partly set (%d of 12)", set);
    EG_REQUIRE(set == (variant == 1 ? 12 : 0), EG_ERR_BAD_ARG, "eg_prior_encoder: variant=%d with %d memory pointers", variant, set);
    EgiPriorW w;
    memset(&w, 0, sizeof(w));
    w.w1 = conv[0]; w.b1 = conv[1]; w.s1 = conv[2]; w.t1 = conv[3]; w.w2 = conv[4]; w.b2 = conv[5]; w.s2 = conv[6]; w.t2 = conv[7];
    if (variant == 1) {
        const int pl = frames - prior_frames, lim = prior_frames < pl ? (prior_frames < 64 ? prior_frames : 64) : (pl < 64 ? pl : 64);
        EG_REQUIRE(chunk >= 1 && chunk <= lim, EG_ERR_BAD_ARG, "eg_prior_encoder: chunk=%d outside 1..min(prior_frames, frames - prior_frames, 64) = %d",
                   chunk, lim);
        EG_REQUIRE(tm_mem && tm_pe && tm_gram, EG_ERR_BAD_ARG, "eg_prior_encoder: the memory variant needs tm_mem, tm_pe and tm_gram");
        w.sp_w0 = mem[0]; w.sp_b0 = mem[1]; w.sp_w1 = mem[2]; w.sp_b1 = mem[3];
        w.tc_w0 = mem[4]; w.tc_b0 = mem[5]; w.tc_w1 = mem[6]; w.tc_b1 = mem[7];
        w.tm_w0 = mem[8]; w.tm_b0 = mem[9]; w.tm_w1 = mem[10]; w.tm_b1 = mem[11];
    }
    return egi_prior_encoder(prior, w, cat, tm_mem, tm_pe, tm_gram, batch, prior_frames, frames, d, dpad, chunk, variant,
                             (hipStream_t)stream);
}

extern "C" int eg_embedding(const int64_t* idx, const float* table, float* out, void* images, void* zero_line, int32_t rows, int32_t dim, int32_t ld,
                            int32_t n_words, void* stream) {
    EG_REQUIRE(idx && table && out, EG_ERR_BAD_ARG, "eg_embedding: null pointer");
    EG_REQUIRE(rows > 0 && dim > 0 && n_words > 0, EG_ERR_BAD_ARG, "eg_embedding: rows=%d dim=%d n_words=%d", rows, dim, n_words);
    EG_REQUIRE((dim & 3) == 0, EG_ERR_ALIGN, "eg_embedding: dim=%d %% 4 != 0", dim);
    EG_REQUIRE(ld >= dim && (ld & 3) == 0, EG_ERR_ALIGN, "eg_embedding: ld=%d < dim=%d or ld %% 4 != 0", ld, dim);
    EG_REQUIRE(images || !zero_line, EG_ERR_BAD_ARG, "eg_embedding: zero_line without images");
    if (!images) return egi_embedding(idx, table, out, rows, dim, ld, n_words, (hipStream_t)stream);
    EG_REQUIRE((ld & 63) == 0, EG_ERR_ALIGN, "eg_embedding: images need ld %% 64 == 0 (ld=%d)", ld);
    return egi_embedding_img(idx, table, out, images, zero_line, rows, dim, ld, n_words, (hipStream_t)stream);
}

extern "C" int eg_small_linear(const float* x, int32_t ldx, const float* w, const float* bias, float* y, int32_t ldy, int32_t n, int32_t in,
                               int32_t out, void* stream) {
    EG_REQUIRE(x && w && bias && y, EG_ERR_BAD_ARG, "eg_small_linear: null pointer");
    EG_REQUIRE(n > 0 && n <= 65535 && in > 0 && out > 0 && ldx >= in && ldy >= out, EG_ERR_BAD_ARG, "eg_small_linear: n=%d in=%d out=%d ldx=%d ldy=%d", n,
               in, out, ldx, ldy);
    return egi_small_linear(x, ldx, w, bias, y, ldy, n, in, out, (hipStream_t)stream);
}

extern "C" int eg_conv_transpose1d(const float* x, const float* w, const float* bias, const float* scale, const float* shift, float* y, int32_t n,
                                   int32_t cin, int32_t cout, int32_t lin, void* stream) {
    EG_REQUIRE(x && w && bias && y, EG_ERR_BAD_ARG, "eg_conv_transpose1d: null pointer");
    EG_REQUIRE(scale && shift, EG_ERR_BAD_ARG, "eg_conv_transpose1d: scale and shift are required");
    EG_REQUIRE(n > 0 && n <= 65535 && cin > 0 && cout > 0 && lin > 0 && lin <= (1 << 29), EG_ERR_BAD_ARG, "eg_conv_transpose1d: n=%d cin=%d cout=%d lin=%d", n,
               cin, cout, lin);
    return egi_convt1d(x, w, bias, scale, shift, y, n, cin, cout, lin, (hipStream_t)stream);
}
