// Shared device/host helpers for libemogest_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <atomic>
#include "emogest.h"

// No packed-fp32 VALU (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32) in any kernel of the library: on MI355X a v_pk_fma_f32 whose operand
// is routed by op_sel / op_sel_hi returns wrong lanes while another wave issues MFMAs on the same SIMD (tools/hazard_probe.hip,
// profiles/r02_hazard_probe.txt); hipcc forms exactly that instruction from `float4 * scalar` code.  The target feature is
// switched off for the whole device compilation by __graft_entry__.DEVICE_FLAGS (a per-function `#pragma clang attribute target(...)`
// was measured in round 3: it leaves the HIP headers' inline device functions with a different feature set, LLVM then refuses to
// inline them, and the convolutions lose 8-36 %); tests/test_isa_gate.py disassembles the built library and fails on any packed-fp32 VALU.

typedef float f4 __attribute__((ext_vector_type(4)));
typedef short bf8 __attribute__((ext_vector_type(8)));   // 8 bf16 (one 16x16x32 MFMA operand)

#define EG_WAVE 64

void eg_set_error(const char* fmt, ...);

#define EG_REQUIRE(cond, code, ...)                      \
    do {                                                 \
        if (!(cond)) {                                   \
            eg_set_error(__VA_ARGS__);                   \
            return (code);                               \
        }                                                \
    } while (0)

// Launch check without synchronising (Guideline 9: nothing blocking in a launch function).  Every kernel launch of the library passes
// through here: the counter behind eg_launch_count() (launches per step of a training / inference pass, reported by bench.py).
extern std::atomic<long long> g_eg_launches;
extern bool g_eg_launch_hist;                   // EG_LAUNCH_HIST=1: also count launches by label (eg_launch_histogram: a diagnostic, off by default)
void egi_count_launch(const char* what);
static inline int eg_check_launch(const char* what) {
    g_eg_launches.fetch_add(1, std::memory_order_relaxed);
    if (g_eg_launch_hist) egi_count_launch(what);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        eg_set_error("%s: %s", what, hipGetErrorString(e));
        return EG_ERR_HIP;
    }
    return EG_OK;
}

// Opt a kernel into more than 64 KB of dynamic LDS.  The attribute is per device, so it is tracked per (kernel, device) under a
// mutex (generator.hip); the HIP status is checked and surfaced as EG_ERR_HIP.  Called from launch functions: cheap after the
// first call, and the first call happens in the host's warm-up pass, outside any stream capture.
int eg_ensure_dynamic_lds(const void* kernel, size_t bytes, const char* who);
#define EG_HIP_TRY(expr, what)                                                         \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) {                                                        \
            eg_set_error("%s: %s", (what), hipGetErrorString(_e));                     \
            return EG_ERR_HIP;                                                         \
        }                                                                              \
    } while (0)

static inline bool eg_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline int64_t eg_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
static inline int eg_cdiv(int a, int b) { return (a + b - 1) / b; }

// ---- device helpers ------------------------------------------------------------------------
// The cross-fade of one overlap element, shared by the roll-out's hand-off (misc.hip) and the stream's (stream.hip) so that the two cannot
// drift: (1 - a) * old + a * fresh with a = alpha[j] (alpha == nullptr: (j + 1) / (P + 1)) as two rounded products and one rounded sum --
// no v_fma here, whatever the translation unit's default: the arithmetic a host restatement in fp32 reproduces bit for bit.
__device__ __forceinline__ float handoff_blend(const float* __restrict__ alpha, int j, int P, float old, float fresh) {
#pragma clang fp contract(off)
    const float a = alpha ? alpha[j] : (float)(j + 1) / (float)(P + 1);
    const float keep = (1.f - a) * old, take = a * fresh;
    return keep + take;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// Sum over the 16 lanes of a DPP row (lanes with the same lane >> 4); every lane of the row gets the total.  Same values, bit for bit, as the chain
// s += __shfl_xor(s, 1); ... 2; ... 4; ... 8 it replaces: the quad permutations ARE lane ^ 1 and lane ^ 2, and once the lanes of a quad (then of a
// half row) hold one value, the half-row mirror (i -> 7 - i) and the row mirror (i -> 15 - i) deliver the same partner value as lane ^ 4 and lane ^ 8.
// Four VALU moves instead of four trips through the LDS crossbar (ds_bpermute) per value.
template <int CTRL> __device__ __forceinline__ float dpp_move(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row16_sum(float s) {
    s += dpp_move<0xB1>(s);         // quad_perm [1, 0, 3, 2]
    s += dpp_move<0x4E>(s);         // quad_perm [2, 3, 0, 1]
    s += dpp_move<0x141>(s);        // row_half_mirror
    s += dpp_move<0x140>(s);        // row_mirror
    return s;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// fp32 -> (hi, lo) bf16 split: hi = rne(x), lo = rne(x - hi).  x - hi is exact in fp32.
__device__ __forceinline__ unsigned short f32_to_bf16_rne(float x) {
    unsigned int u = __float_as_uint(x);
    // NaN stays NaN: the rounding add below carries a full mantissa into the sign (0x7FFFFFFF -> -0) and turns a small payload into inf
    // (0x7F800001 -> 0x7F80); keep sign and high payload, set the quiet bit.  Finite values and inf are untouched.
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (unsigned short)((u >> 16) | 0x0040u);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float(((unsigned int)h) << 16); }

// split 8 consecutive fp32 into bf16 (hi, lo) octets with the hardware packed convert (v_cvt_pk_bf16_f32):
// 2 cvt + shl + and + packed sub per pair of floats.
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
template <bool WANT_LO>
__device__ __forceinline__ void split_octet(const f4& v0, const f4& v1, bf8& hi, bf8& lo) {
    u32x4_t h, l;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const f32x2_t x = {p < 2 ? v0[2 * p] : v1[2 * p - 4], p < 2 ? v0[2 * p + 1] : v1[2 * p - 3]};
        const unsigned hu = __builtin_bit_cast(unsigned, __builtin_convertvector(x, bf16x2_t));
        h[p] = hu;
        if (WANT_LO) {
            const f32x2_t r = {x[0] - __uint_as_float(hu << 16), x[1] - __uint_as_float(hu & 0xffff0000u)};
            l[p] = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2_t));
        }
    }
    hi = __builtin_bit_cast(bf8, h);
    if (WANT_LO) lo = __builtin_bit_cast(bf8, l);
}

// ---- counter-based dropout mask (train.hip: eg_dropout; attention.hip: the probabilities' dropout of Modules.py:21) -------------------------
// keep(i) = hash(seed, counter i) >= p * 2^32: nothing is stored, the backward pass recomputes the mask from the same (seed, counter).
__device__ __forceinline__ unsigned int mix32(unsigned int h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
// `epoch` (optional, device resident): a per-step counter mixed into the seed, so that a step replayed from a captured hipGraph -- whose host
// scalars (seed, offset) are frozen -- still draws a fresh mask every replay (train/graph.py increments it inside the graph).
__device__ __forceinline__ unsigned int dropout_seed(unsigned int seed, const int* __restrict__ epoch) {
    return epoch ? seed ^ mix32((unsigned int)*epoch * 0x9E3779B9u + 0x7F4A7C15u) : seed;
}
__device__ __forceinline__ bool dropout_keep(unsigned int seed, unsigned long long ctr, unsigned int thr) {
    return mix32(mix32((unsigned int)ctr ^ seed) + (unsigned int)(ctr >> 32) * 0x9E3779B9u + 0x6A09E667u) >= thr;
}
struct EgDropout {              // p = 0 (thr = 0): identity
    unsigned int thr = 0, seed = 0;
    float inv_keep = 1.f;
    unsigned long long offset = 0;
    const int* epoch = nullptr;
};

// ---- optional launch profiler (generator.hip) ----------------------------------------------------------------
// XCD-aware tile order for 2-D tile grids.  Workgroups are dealt round-robin to the 8 XCDs in launch order (x fastest), each
// XCD with its own L2.  Give XCD k a contiguous run of logical tile ids (y fastest inside the run) so that the tiles sharing a
// row panel (same bx: the activations) land on one XCD and hit its L2, instead of every XCD fetching every panel across the
// fabric (measured before this mapping: 5-6x the algorithmic read bytes per GEMM launch at the memory-side counters).
__device__ __forceinline__ void xcd_tile(int& bx, int& by) {
    const int gx = gridDim.x, gy = gridDim.y, total = gx * gy;
    const int lin = blockIdx.y * gx + blockIdx.x;
    const int xcd = lin & 7, idx = lin >> 3;
    const int q = total >> 3, r = total & 7;
    const int log = xcd * q + (xcd < r ? xcd : r) + idx;      // XCDs below r own q+1 tiles
    bx = log / gy;
    by = log - bx * gy;
}

// s_waitcnt as real instructions (builtins, not inline asm) so that the compiler's own wait insertion accounts for them
template <int N> __device__ __forceinline__ void wait_vmcnt_imm() {
    // s_waitcnt vmcnt(N) with expcnt / lgkmcnt left at their maxima (gfx9 encoding: vmcnt[3:0] | expcnt<<4 | lgkmcnt<<8 | vmcnt[5:4]<<14)
    __builtin_amdgcn_s_waitcnt((N & 15) | 0x70 | 0xF00 | ((N >> 4) << 14));
}
__device__ __forceinline__ void wait_lgkmcnt0() { __builtin_amdgcn_s_waitcnt(0xC07F); }
// raw workgroup barrier (no implied vmcnt/lgkmcnt drain).  The s_barrier builtin is "no memory" at IR level, so the empty asm
// statements keep the optimiser from moving LDS reads / LDS-DMA issues across it.
__device__ __forceinline__ void wg_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

struct EgProfScope {
    int slot;
    hipStream_t st;
    EgProfScope(int64_t tag, double flops, hipStream_t s);
    void workgroups(int n);          // workgroups of the launch (0 = not recorded: a grid that covers the chip)
    ~EgProfScope();
};

// ---- internal (C++ linkage) operands of the fused CVAE sample (misc.hip: cvae_sample_fused_kernel), filled by generator.hip ------------
struct EgiCvaeFused {
    const float *y = nullptr, *z = nullptr;                          // [n][8] labels, [n][32] latent draws
    const float *lin_w[4] = {}, *lin_b[4] = {};                      // Posterior_Y_embedding.0 / .2, fusion_z_posterior.0 / .2
    const float *t_w[2] = {}, *t_b[2] = {}, *t_s[2] = {}, *t_t[2] = {};      // ConvTranspose 4->8, 8->16: weight, bias, BN scale, BN shift
    const float *c_w[3] = {}, *c_b[3] = {}, *c_s[2] = {}, *c_t[2] = {};      // Conv 16->32, 32->F, F->F (the last one plain)
    float* out = nullptr;                                           // [n][F][L]
    int F = 0, L = 0, T = 0;                                        // frames, d_model, tile of the L axis (set by the launch function)
};

// ---- internal (C++ linkage) product descriptor shared by gemm.hip and generator.hip --------------------------------
struct EgiLinear {
    const float* x = nullptr; int lda = 0;                          // fp32 input, or ...
    const void* ximg = nullptr; int xK = 0, xk0 = 0;                // ... pre-split images of width xK, this product's K range starts at xk0
    const float* w = nullptr; int ldw = 0; const float* bias = nullptr;
    const float* res1 = nullptr; const float* res2 = nullptr; int ldr = 0;
    float* y = nullptr; int ldc = 0;
    void* yimg = nullptr; int yK = 0, yk0 = 0;                      // optional pre-split output images of width yK at column offset yk0
    int m = 0, n = 0, k = 0, relu = 0, a_shift = 0, a_seq = 1, precision = 0;
    int shared_chip = 0;                                            // the caller keeps other work resident (several batches in flight): tile for CU time, not latency
    int xs_shift = 0, xs_period = 1; const void* xzero = nullptr;   // pre-split input only: causal two-tap product -- k = 2 * tap width, W = [N][tap 0 | tap 1]; K steps of tap 0 read row r - xs_shift (zero where r mod xs_period < xs_shift, from the cleared line xzero of k/2 * 128 bytes)
    int splits = 0; float* partial = nullptr;                       // pre-split input only: split K over `splits` workgroup slices (partial >= splits*m*n floats), fixed-order fold
};
