// Preview frames (include/emogest.h: eg_preview_max_bones, eg_preview_check, eg_preview_raster): stick figures of whole takes, one 8-bit
// picture per frame.  The picture is defined by a formula in single IEEE fp32 operations (the header states it; `coverage` and `blend` below
// are that formula and nothing else computes a pixel), so numpy in float32 reproduces the bytes.
// One workgroup per (frame, band of BAND image rows).  It projects the joints the bones name once into LDS, then its first wave makes one bone
// per lane -- the end points, the reciprocal of the squared length, the bounding box -- and keeps, by ballot so that the order of the bones
// survives, the list of the bones whose box touches the band.  A figure covers a few percent of a picture, so most bands have a short list.
// The band is cut into blocks of 8 rows x 128 pixels, which the waves take in turn.  A block is composited in the wave's own LDS tile, one
// packed word per pixel: for every listed bone whose box reaches the block the wave walks the box's columns eight at a time (lane = row and
// column of an 8 x 8 step), so the arithmetic follows the bones' boxes, not the picture's area -- a run-per-lane version that evaluated every
// listed bone on all 16 pixels of every lane was 2.5-3.0 x slower at 240 x 320 (profiles/preview_bench_line_run_per_lane.json).  Integer compositing in bone order; a pixel the bone does not
// reach (q = 0) keeps its value.  Then every lane reads its run of PX = 16 pixels back as four 16-byte LDS reads, and the 48 bytes leave as
// three 16-byte stores (hwc) or one per plane (chw): a row of a block is one 128-byte line of a plane.  The boxes only skip work: they are
// grown by more than the formula's rounding can move a pixel's distance, so a skipped pixel has q = 0 by the formula too.
// A frame behind the row's count writes zeros without reading a joint.  No atomics, no memset; the grid depends on (rows, T, H, W) only.
#include "rows.h"
#include <math.h>
#include <string.h>

// What the bit-for-bit definition needs from the compilation, beyond no contraction: fp32 subnormals kept (hipcc's default for gfx9: no
// -fgpu-flush-denormals-to-zero, which __graft_entry__ does not pass) and a correctly rounded 1 / x and sqrt (hipcc's default,
// -fhip-fp32-correctly-rounded-divide-sqrt).  The "degenerate" case of tests/preview_cases.py has a bone whose squared length is subnormal
// and fails on a build that flushes.
#pragma clang fp contract(off)

namespace {

constexpr int MAXB = EG_PREVIEW_MAX_BONES;
constexpr int MAXU = 2 * MAXB;                          // distinct joints the bones can name
constexpr int THREADS = 256;
constexpr int PX = 16;                                  // consecutive pixels of one thread
constexpr int BAND = 32;                                // image rows of one workgroup
constexpr int BLOCK_ROWS = 8, BLOCK_RUNS = 8;           // a wave's block: 8 rows of 8 runs (128 pixels), one run per lane
constexpr int BLOCK_PIXELS = BLOCK_RUNS * PX;            // 128 pixels across
constexpr int PITCH = BLOCK_PIXELS + 8;                 // words per row of a wave's LDS tile: the eight rows of a column step start 8 banks apart
static_assert(BLOCK_ROWS * BLOCK_RUNS == EG_WAVE && BAND % BLOCK_ROWS == 0 && PITCH % 4 == 0, "one run per lane; whole blocks in a band");
constexpr int W_BONES = 0, W_USED = 1, W_BACKGROUND = 2, W_JOINT = 4, W_A = W_JOINT + MAXU, W_B = W_A + MAXB, W_COLOUR = W_B + MAXB;
static_assert(W_COLOUR + MAXB == EG_PREVIEW_TABLE_WORDS && MAXB <= EG_WAVE, "the table's layout; one bone per lane of the first wave");

enum { P_AX, P_AY, P_EX, P_EY, P_INV, P_X0, P_X1, P_Y0, P_Y1, P_COUNT };

struct Args {
    const float* joints;                                // [rows, T, J, 3]
    const int* table;                                   // device, EG_PREVIEW_TABLE_WORDS
    const int* frames;                                  // device [rows / draws] or null
    uint8_t* out;
    float m[8];                                         // M00 M01 M02 M10 M11 M12 c0 c1
    float radius;
    int T, J, H, W, draws, frame_unit, segs, cols, tiles;  // 16-pixel runs of a row, blocks across a band, bands of a picture
};

// q of the header's formula for the pixel centre (X, ay + wy); reach = radius + 0.5.
__device__ __forceinline__ unsigned coverage(float X, float wy, float ax, float ex, float ey, float inv, float reach) {
    const float wx = X - ax;
    const float s = (wx * ex + wy * ey) * inv;
    float t = s < 0.f ? 0.f : s;
    t = t > 1.f ? 1.f : t;
    const float dx = wx - t * ex, dy = wy - t * ey;
    const float a = reach - __builtin_sqrtf(dx * dx + dy * dy);
    return a >= 1.f ? 255u : a > 0.f ? (unsigned)(int)(a * 255.f + 0.5f) : 0u;
}

__device__ __forceinline__ unsigned blend(unsigned c, unsigned colour, unsigned q) { return (c * (255u - q) + colour * q + 127u) / 255u; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool ALIGNED>
__device__ __forceinline__ void store16(uint8_t* p, const u32x4_t v) {
    if (ALIGNED) *reinterpret_cast<u32x4_t*>(p) = v;
    else __builtin_memcpy(p, &v, 16);                   // a row of a picture whose width is no multiple of 16 starts on any byte
}

// Sixteen values of one channel, one byte each.
template <bool ALIGNED>
__device__ __forceinline__ void store_plane(uint8_t* p, const unsigned (&c)[PX], int npx) {
    if (npx == PX) {
        u32x4_t v;
#pragma unroll
        for (int w = 0; w < 4; ++w) v[w] = c[4 * w] | (c[4 * w + 1] << 8) | (c[4 * w + 2] << 16) | (c[4 * w + 3] << 24);
        store16<ALIGNED>(p, v);
    } else {
#pragma unroll
        for (int i = 0; i < PX; ++i)
            if (i < npx) p[i] = (uint8_t)c[i];
    }
}

template <int LAYOUT, bool ALIGNED>
__global__ __launch_bounds__(THREADS) void preview_raster_kernel(const Args a) {
    __shared__ float s_u[MAXU], s_v[MAXU];
    __shared__ float s_p[P_COUNT][MAXB];
    __shared__ unsigned s_colour[MAXB];
    __shared__ int s_listed;
    __shared__ __attribute__((aligned(16))) unsigned s_pix[THREADS / EG_WAVE][BLOCK_ROWS][PITCH];
    const int tid = threadIdx.x;
    int blk = blockIdx.x;                               // a frame's tiles are neighbours: they read the same joints
    const int tile = blk % a.tiles; blk /= a.tiles;
    const int t = blk % a.T, b = blk / a.T;
    const int n = egi_valid_frames(a.frames, b / a.draws, a.frame_unit, a.T);
    const bool valid = t < n;                           // the same for the whole workgroup
    const int y_lo = tile * BAND, y_hi = min(a.H, y_lo + BAND);
    const long long frame = (long long)b * a.T + t;
    if (valid) {
        // every table word this thread can need, loaded together (all inside the table, whatever it holds): one trip to memory, not three
        const int nb = clampi(a.table[W_BONES], 0, MAXB), nu = clampi(a.table[W_USED], 0, MAXU), bone = tid & (MAXB - 1);
        const int w_joint = a.table[W_JOINT + (tid & (MAXU - 1))], w_a = a.table[W_A + bone], w_b = a.table[W_B + bone], w_colour = a.table[W_COLOUR + bone];
        if (tid < nu) {
            const float* p = a.joints + (frame * a.J + clampi(w_joint, 0, a.J - 1)) * 3;
            const float x = p[0], y = p[1], z = p[2];
            s_u[tid] = ((a.m[0] * x + a.m[1] * y) + a.m[2] * z) + a.m[6];
            s_v[tid] = ((a.m[3] * x + a.m[4] * y) + a.m[5] * z) + a.m[7];
        }
        __syncthreads();
        if (tid < EG_WAVE) {
            bool hit = false;
            float ax = 0.f, ay = 0.f, ex = 0.f, ey = 0.f, inv = 0.f, x0 = 0.f, x1 = 0.f, y0 = 0.f, y1 = 0.f;
            if (tid < nb && nu > 0) {
                const int ia = clampi(w_a, 0, nu - 1), ib = clampi(w_b, 0, nu - 1);
                ax = s_u[ia]; ay = s_v[ia];
                const float bx = s_u[ib], by = s_v[ib];
                ex = bx - ax; ey = by - ay;
                const float l2 = ex * ex + ey * ey;
                inv = l2 > 0.f ? 1.f / l2 : 0.f;
                // An end that is not finite makes every q of the bone 0.  Otherwise the point the formula measures to lies between the
                // ends up to its rounding, at most (2 (H + W) + 8 big) 2^-24: the box is grown by sixteen times that on top of radius + 1.
                const bool finite = __builtin_isfinite(ax) && __builtin_isfinite(ay) && __builtin_isfinite(bx) && __builtin_isfinite(by);
                const float big = fmaxf(fmaxf(fabsf(ax), fabsf(ay)), fmaxf(fabsf(bx), fabsf(by)));
                const float grow = (a.radius + 1.f) + (big + (float)(a.H + a.W)) * 0x1p-20f;
                x0 = fminf(ax, bx) - grow; x1 = fmaxf(ax, bx) + grow;
                y0 = fminf(ay, by) - grow; y1 = fmaxf(ay, by) + grow;
                hit = finite && y1 >= (float)y_lo && y0 <= (float)y_hi && x1 >= 0.f && x0 <= (float)a.W;
            }
            const unsigned long long mask = __ballot(hit);
            if (hit) {
                const int pos = __popcll(mask & ((1ull << tid) - 1ull));                // bones keep their order
                s_p[P_AX][pos] = ax; s_p[P_AY][pos] = ay; s_p[P_EX][pos] = ex; s_p[P_EY][pos] = ey; s_p[P_INV][pos] = inv;
                s_p[P_X0][pos] = x0; s_p[P_X1][pos] = x1; s_p[P_Y0][pos] = y0; s_p[P_Y1][pos] = y1;
                s_colour[pos] = (unsigned)w_colour;
            }
            if (tid == 0) s_listed = __popcll(mask);
        }
        __syncthreads();
    }
    // A wave takes the band's blocks in turn.  A block's picture is built in the wave's own LDS tile, one packed word per pixel: for every
    // listed bone the wave walks the columns of the block that the bone's box reaches, eight at a time with one row per eight lanes, so the
    // work follows the bones and not the block's area; lanes touch different pixels and the bones come in order, so nothing races.
    const int lane = tid & (EG_WAVE - 1), wave = tid / EG_WAVE;
    const int ry = lane / BLOCK_RUNS, rx = lane % BLOCK_RUNS;
    const unsigned bg = valid ? (unsigned)a.table[W_BACKGROUND] & 0xffffffu : 0u;
    unsigned (*pix)[PITCH] = s_pix[wave];
    for (int block = wave; block < a.cols * (BAND / BLOCK_ROWS); block += THREADS / EG_WAVE) {
        const int by0 = y_lo + (block / a.cols) * BLOCK_ROWS, bx0 = (block % a.cols) * BLOCK_PIXELS;
        if (by0 >= y_hi) continue;
        const int y = by0 + ry, px0 = bx0 + rx * PX;
        {
            const u32x4_t fill = {bg, bg, bg, bg};
#pragma unroll
            for (int i = 0; i < PX; i += 4) *reinterpret_cast<u32x4_t*>(&pix[ry][rx * PX + i]) = fill;
        }
        __builtin_amdgcn_wave_barrier();
        if (valid) {
            const int listed = s_listed;
            const float Y = (float)y + 0.5f, reach = a.radius + 0.5f;
            const float bxl = (float)bx0, bxr = (float)min(bx0 + BLOCK_PIXELS, a.W), byl = (float)by0, byr = (float)(by0 + BLOCK_ROWS);
            for (int k = 0; k < listed; ++k) {
                const float y0 = s_p[P_Y0][k], y1 = s_p[P_Y1][k];
                const float fx0 = fmaxf(s_p[P_X0][k], bxl), fx1 = fminf(s_p[P_X1][k], bxr);       // inside [0, 2048]: safe to convert
                if (!(fx0 <= fx1 && y1 >= byl && y0 <= byr)) continue;                              // the same for every lane
                const int x_lo = max((int)fx0 - 1, bx0), x_hi = min((int)fx1 + 1, (int)bxr);       // centres x + 0.5 inside the box, and more
                const bool in_rows = Y >= y0 && Y <= y1;
                const float ax = s_p[P_AX][k], ex = s_p[P_EX][k], ey = s_p[P_EY][k], inv = s_p[P_INV][k];
                const float wy = Y - s_p[P_AY][k];
                const unsigned colour = s_colour[k], c0 = colour & 255u, c1 = (colour >> 8) & 255u, c2 = (colour >> 16) & 255u;
                for (int x = x_lo + rx; x < x_hi; x += BLOCK_RUNS) {
                    const unsigned q = in_rows ? coverage((float)x + 0.5f, wy, ax, ex, ey, inv, reach) : 0u;
                    if (q) {
                        const unsigned c = pix[ry][x - bx0];
                        pix[ry][x - bx0] = blend(c & 255u, c0, q) | (blend((c >> 8) & 255u, c1, q) << 8) | (blend(c >> 16, c2, q) << 16);
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (y >= y_hi || px0 >= a.W) continue;          // a row or a run outside the picture
        const int npx = min(PX, a.W - px0);
        unsigned c[3][PX];
#pragma unroll
        for (int i = 0; i < PX; i += 4) {
            const u32x4_t v = *reinterpret_cast<const u32x4_t*>(&pix[ry][rx * PX + i]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                c[0][i + e] = v[e] & 255u; c[1][i + e] = (v[e] >> 8) & 255u; c[2][i + e] = v[e] >> 16;
            }
        }
        if (LAYOUT == EG_PREVIEW_CHW) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) store_plane<ALIGNED>(a.out + ((frame * 3 + ch) * a.H + y) * a.W + px0, c[ch], npx);
        } else {
            uint8_t* p = a.out + ((frame * a.H + y) * a.W + px0) * 3;
            if (npx == PX) {
#pragma unroll
                for (int w4 = 0; w4 < 3; ++w4) {            // byte m of the 48 is channel m % 3 of pixel m / 3
                    u32x4_t v;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const int m = 16 * w4 + 4 * w;
                        v[w] = c[m % 3][m / 3] | (c[(m + 1) % 3][(m + 1) / 3] << 8) | (c[(m + 2) % 3][(m + 2) / 3] << 16) | (c[(m + 3) % 3][(m + 3) / 3] << 24);
                    }
                    store16<ALIGNED>(p + 16 * w4, v);
                }
            } else {
#pragma unroll
                for (int i = 0; i < PX; ++i)
                    if (i < npx) {
                        p[3 * i] = (uint8_t)c[0][i]; p[3 * i + 1] = (uint8_t)c[1][i]; p[3 * i + 2] = (uint8_t)c[2][i];
                    }
            }
        }
    }
}

int check_bones(const char* who, const int32_t* bones, int n_bones, int J) {
    EG_REQUIRE(bones, EG_ERR_BAD_ARG, "%s: null bones", who);
    EG_REQUIRE(n_bones >= 1 && n_bones <= MAXB, EG_ERR_UNSUPPORTED, "%s: bones=%d (1..EG_PREVIEW_MAX_BONES = %d)", who, n_bones, MAXB);
    EG_REQUIRE(J >= 1, EG_ERR_BAD_ARG, "%s: J=%d joints (need >= 1)", who, J);
    for (int k = 0; k < n_bones; ++k)
        for (int e = 0; e < 2; ++e)
            EG_REQUIRE(bones[2 * k + e] >= 0 && bones[2 * k + e] < J, EG_ERR_BAD_ARG, "%s: bone %d names joint %d of J=%d (0..%d)", who, k,
                       bones[2 * k + e], J, J - 1);
    return EG_OK;
}

}  // namespace

extern "C" int32_t eg_preview_max_bones(void) { return MAXB; }

extern "C" int eg_preview_check(const int32_t* bones, int32_t n_bones, int32_t J) { return check_bones("eg_preview_check", bones, n_bones, J); }

extern "C" int eg_preview_raster(const float* joints, int32_t rows, int32_t T, int32_t J, const int32_t* bones, int32_t n_bones,
                                 const int32_t* d_table, const float* camera, float radius, int32_t H, int32_t W, int32_t layout,
                                 int32_t draws, int32_t frame_unit, const int32_t* d_frames, uint8_t* out, void* stream) {
    const char* who = "eg_preview_raster";
    EG_REQUIRE(joints, EG_ERR_BAD_ARG, "%s: null joints", who);
    EG_REQUIRE(out, EG_ERR_BAD_ARG, "%s: null out", who);
    EG_REQUIRE(d_table, EG_ERR_BAD_ARG, "%s: null d_table", who);
    EG_REQUIRE(camera, EG_ERR_BAD_ARG, "%s: null camera", who);
    EG_REQUIRE(eg_aligned16(joints) && eg_aligned16(out) && eg_aligned16(d_table), EG_ERR_ALIGN, "%s: joints / out / d_table not 16-byte aligned", who);
    EG_REQUIRE(rows >= 1 && T >= 1, EG_ERR_BAD_ARG, "%s: rows=%d frames=%d (need >= 1)", who, rows, T);
    int rc = check_bones(who, bones, n_bones, J);
    if (rc != EG_OK) return rc;
    EG_REQUIRE(H >= EG_PREVIEW_MIN_SIZE && H <= EG_PREVIEW_MAX_SIZE && W >= EG_PREVIEW_MIN_SIZE && W <= EG_PREVIEW_MAX_SIZE, EG_ERR_UNSUPPORTED,
               "%s: height=%d width=%d (each %d..%d)", who, H, W, EG_PREVIEW_MIN_SIZE, EG_PREVIEW_MAX_SIZE);
    EG_REQUIRE(radius >= EG_PREVIEW_MIN_RADIUS && radius <= EG_PREVIEW_MAX_RADIUS, EG_ERR_UNSUPPORTED, "%s: radius=%g pixels (%g..%g)", who,
               (double)radius, (double)EG_PREVIEW_MIN_RADIUS, (double)EG_PREVIEW_MAX_RADIUS);
    for (int i = 0; i < 8; ++i) EG_REQUIRE(isfinite(camera[i]), EG_ERR_BAD_ARG, "%s: camera[%d]=%g is not finite", who, i, (double)camera[i]);
    EG_REQUIRE(layout == EG_PREVIEW_HWC || layout == EG_PREVIEW_CHW, EG_ERR_BAD_ARG, "%s: layout=%d (EG_PREVIEW_HWC or EG_PREVIEW_CHW)", who, layout);
    rc = egi_check_rows(who, rows, T, nullptr, d_frames, false, draws, frame_unit, 0, "");
    if (rc != EG_OK) return rc;
    const int segs = eg_cdiv(W, PX), cols = eg_cdiv(segs, BLOCK_RUNS);
    const long long tiles = eg_cdiv(H, BAND), grid = (long long)rows * T * tiles;
    EG_REQUIRE(grid <= 0x7fffffffll && (long long)rows * T * J * 3 < (1ll << 40), EG_ERR_UNSUPPORTED,
               "%s: rows=%d x frames=%d x %d x %d pixels, J=%d: grid / index range", who, rows, T, H, W, J);
    Args a = {joints, d_table, d_frames, out, {}, radius, T, J, H, W, draws, frame_unit, segs, cols, (int)tiles};
    memcpy(a.m, camera, sizeof a.m);
    const dim3 g((unsigned)grid), blk(THREADS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool aligned = W % PX == 0;                   // then every 16-pixel run of every plane and row starts on 16 bytes
    if (layout == EG_PREVIEW_CHW) {
        if (aligned) hipLaunchKernelGGL((preview_raster_kernel<EG_PREVIEW_CHW, true>), g, blk, 0, st, a);
        else hipLaunchKernelGGL((preview_raster_kernel<EG_PREVIEW_CHW, false>), g, blk, 0, st, a);
    } else {
        if (aligned) hipLaunchKernelGGL((preview_raster_kernel<EG_PREVIEW_HWC, true>), g, blk, 0, st, a);
        else hipLaunchKernelGGL((preview_raster_kernel<EG_PREVIEW_HWC, false>), g, blk, 0, st, a);
    }
    return eg_check_launch("preview_raster");
}
