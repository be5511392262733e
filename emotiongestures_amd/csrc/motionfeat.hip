// Motion-clip features of whole tracks (include/emogest.h: eg_motion_window_rows): PoseEncoderConv.net of MotionAE on every 34-frame window of
// ragged tracks with R takes each, in one launch.
//   * A workgroup owns a run of run_windows(S) consecutive strided windows of one take; the tail window (start frames[u] - 34, on no stride
//     grid) is a run of its own.  The clip range [c0, c1) clips the run; the window plan is eg_emotion_meta's.
//   * The poses of the run are staged once, channel-major (egi_stage_exact_t: nothing at or beyond frames[u] is read).  Windows that overlap or
//     touch (S < 34) share one contiguous span; windows that do not are staged back to back, 34 frames each ("compact" positions).
//   * conv1 and conv2 (stride 1, no padding) run once per compact position of the run; conv3 (stride 2) and conv4 run per window, in batches
//     of BATCH windows.  A lane owns a position, a wave a group of output channels: 4 windows of 32 / 30 / 14 / 12 positions fill the 64
//     lanes that one window would leave half empty, and the weight reads are wave-uniform 16-byte LDS broadcasts.
//   * Dense form, where the windows of a run overlap so much that it is less work (small strides): output l of conv3 for the window at pose s
//     reads conv2 at s + 2l + k, so it is c3[s + 2l] of ONE stride-1 pass c3[p] = conv3 at p, and output l of conv4 is c4[s + 2l] with
//     c4[p] = sum_k w4[k] c3[p + 2k] -- the windows of one start parity share everything.  Both run once per position of the run and the
//     rows are gathered from c4.  The same terms in the same order per element, hence the same bits as the per-window form.
//   * The weights are staged layer by layer as [ci * k][cout + 4] (the pad spreads the transposing 16-byte writes over the banks); the regions
//     of dead operands are reused (layout below): 162 816 bytes, one workgroup of 8 waves per CU.
// Every output element of every layer: bias, then fmaf per term with ci ascending and k inner, then LeakyReLU -- conv1d_kernel's chain (misc.hip),
// so the rows are bit for bit what four eg_conv1d calls give on host-cut windows, whatever is shared.  Every LDS cell and every output element
// has one owning thread per phase; plain stores, no atomics.
#include "rows.h"

namespace {

constexpr int F = EG_MOTION_WINDOW;                     // 34 -> 32 -> 30 -> 14 -> 12
constexpr int N1 = 32, N2 = 30, N3 = 14, N4 = 12;
constexpr int C1 = 32, C2 = 64, C3 = 64, C4 = 32;
constexpr int MAXD = EG_MOTION_MAX_POSE_DIM;
constexpr int MAXR = EG_TAKE_MAX_DRAWS;
constexpr int MAX_U = 65535;                            // blockIdx.y carries the recording
constexpr int THREADS = 512, WAVES = THREADS / 64;
constexpr int POS = 128;                                // compact positions of conv1 / conv2 in one run: the pitch of a1 and a2
constexpr int XF = EG_MOTION_RUN_FRAMES;                // compact frames of one run
constexpr int XP = XF + 1;                              // pitch of the staged poses: odd, so the transposing stores of a wave (lanes 4 columns apart) spread over 8 banks, not 1
constexpr int BATCH = 8;                                // windows of one conv3 / conv4 pass
constexpr int P3 = BATCH * N3;                          // pitch of a3
static_assert(C4 * N4 == EG_MOTION_ROW_FLOATS && 4 * F == XF && 4 * N1 == POS, "row layout and run geometry");

// LDS layout in floats.  Phase 1: x | W1 | a1.  Phase 2: W2 | a2 (over x), a1 read.  Phase 3: a3 (over W2) | a2 | W3 (over W1, a1) | W4;
// the dense form keeps c3 [64][POS] in a3's place and writes c4 [32][POS] over a2 once conv3 has consumed it.
constexpr int X_OFF = 0;
constexpr int W1_OFF = MAXD * XP;                                   // 17 536
constexpr int A1_OFF = W1_OFF + MAXD * 3 * (C1 + 4);                // 31 360
constexpr int W2_OFF = 0;
constexpr int A3_OFF = 0;
constexpr int A2_OFF = C3 * POS;                                    //  8 192 (>= C3 * P3)
constexpr int W3_OFF = A2_OFF + C2 * POS;                           // 16 384
constexpr int W4_OFF = W3_OFF + C2 * 4 * (C3 + 4);                  // 33 792
constexpr int LDS_FLOATS = W4_OFF + C3 * 3 * (C4 + 4);              // 40 704: 162 816 bytes (phase 1 ends at 35 456)
static_assert(A1_OFF + C1 * POS <= LDS_FLOATS && W1_OFF % 4 == 0 && A1_OFF % 4 == 0, "phase 1 fits, 16-byte aligned regions");
static_assert(W2_OFF + C1 * 3 * (C2 + 4) <= A2_OFF && A2_OFF + C2 * POS <= A1_OFF, "phase 2: W2 and a2 leave a1 alone");
static_assert(W3_OFF >= A2_OFF + C2 * POS && A3_OFF + C3 * P3 <= A2_OFF && A3_OFF + C3 * POS <= A2_OFF && C4 <= C2,
              "phase 3: a3 / c3, a2 / c4, W3, W4 are disjoint");
static_assert(LDS_FLOATS * 4 <= 160 * 1024, "LDS");

// Windows of one run: conv1's compact positions fill POS -- 4 windows of 32 where they are cut apart (S >= 32), (w - 1) * S + 32 <= 128 where
// they share a span; whole batches where there are several.  The staged frames are then at most 4 * 34 = XF, or (w - 1) * S + 34 <= 133.
__host__ __device__ inline int run_windows(int S) {
    const int w = S >= N1 ? POS / N1 : (POS - N1) / S + 1;
    return w > BATCH ? w - w % BATCH : w;
}
__host__ __device__ inline int window_count(int f, int S, int tail) { return (f - F) / S + 1 + (tail && (f - F) % S != 0 ? 1 : 0); }
__host__ __device__ inline int run_count(int f, int S, int tail) {
    const int strided = (f - F) / S + 1, w = run_windows(S);
    return (strided + w - 1) / w + (tail && (f - F) % S != 0 ? 1 : 0);
}

// w [Cout][CK] (PyTorch's [cout][cin][k]) -> ws[ck * (Cout + 4) + co]: four coalesced loads along ck, one 16-byte store.
__device__ __forceinline__ void stage_weights(float* __restrict__ ws, const float* __restrict__ w, int CK, int Cout, int tid) {
    const int wp = Cout + 4, n = (Cout >> 2) * CK;
    for (int i = tid; i < n; i += THREADS) {
        const int c4 = i / CK, ck = i - c4 * CK;
        const float* src = w + (size_t)(c4 * 4) * CK + ck;
        f4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = src[(size_t)r * CK];
        *reinterpret_cast<f4*>(ws + ck * wp + c4 * 4) = v;
    }
}

// One layer over `count` compact output positions: work items (64 positions, COG output channels) dealt to the waves; lane q reads its K taps
// of input channel ci at in[ci * pitch + index(q) + k * TS] and hands the finished COG sums to store(q, co, value).
template <int K, int TS, int COG, int COUT, bool LEAKY, class Index, class Store>
__device__ __forceinline__ void conv_pass(const float* __restrict__ in, int pitch, const float* __restrict__ ws, const float* __restrict__ bias,
                                          int Cin, int count, int wave, int lane, Index index, Store store) {
    constexpr int WP = COUT + 4, GROUPS = COUT / COG;
    const int items = ((count + 63) >> 6) * GROUPS;
    for (int item = wave; item < items; item += WAVES) {            // wave-uniform
        const int tile = item / GROUPS, co0 = (item - tile * GROUPS) * COG;
        const int q = tile * 64 + lane;
        const bool live = q < count;
        const float* xp = in + index(live ? q : 0);                 // a lane past the end computes position 0 and stores nothing
        const float* wq = ws + co0;
        f4 acc[COG / 4];
#pragma unroll
        for (int j = 0; j < COG / 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[j][r] = bias[co0 + j * 4 + r];
        for (int ci = 0; ci < Cin; ++ci) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float xv = xp[k * TS];
#pragma unroll
                for (int j = 0; j < COG / 4; ++j) {
                    const f4 wv = *reinterpret_cast<const f4*>(wq + k * WP + j * 4);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[j][r] = fmaf(wv[r], xv, acc[j][r]);
                }
            }
            xp += pitch;
            wq += K * WP;
        }
        if (live) {
#pragma unroll
            for (int j = 0; j < COG / 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float s = acc[j][r];
                    if (LEAKY) s = s > 0.f ? s : 0.2f * s;
                    store(q, co0 + j * 4 + r, s);
                }
        }
    }
}

struct MotionArgs {
    const float* track;
    const int* meta;                                    // frames | off | C | coff
    const float* w[4];
    const float* b[4];
    float* rows;
    int U, R, Tmax, D, S, tail, maxruns, c0, c1;
};

// blockIdx.y = u, blockIdx.x = r * maxruns + run.  Every early return is workgroup-uniform and precedes the first barrier.
__global__ __launch_bounds__(THREADS) void motion_window_rows_kernel(const MotionArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int u = blockIdx.y, S = a.S, D = a.D;
    const int r = blockIdx.x / a.maxruns, run = blockIdx.x - r * a.maxruns;
    const int f = a.meta[u], coff = a.meta[3 * a.U + u];
    if (f < F || f > a.Tmax) return;                    // the host refused this on its copy: a device table that differs reads nothing
    const int strided = (f - F) / S + 1, W = run_windows(S);
    const bool has_tail = a.tail && (f - F) % S != 0;
    const int n = strided + (has_tail ? 1 : 0), nruns = (strided + W - 1) / W;
    int j0, nw;                                         // the run's first window in the take and its window count
    if (run < nruns) { j0 = run * W; nw = strided - j0 < W ? strided - j0 : W; }
    else if (run == nruns && has_tail) { j0 = strided; nw = 1; }
    else return;
    const long long base = (long long)a.R * coff + (long long)r * n;        // the take's first clip
    const long long lo = (long long)a.c0 - base, hi = (long long)a.c1 - base;      // the clip range in this take's window numbers
    const long long ja = lo > j0 ? lo : j0, jb = hi < j0 + nw ? hi : j0 + nw;
    if (ja >= jb) return;
    j0 = (int)ja;
    nw = (int)(jb - ja);
    const int start0 = j0 == strided ? f - F : j0 * S;  // the tail run is its single window
    float* rows = a.rows + (size_t)(base + j0 - a.c0) * EG_MOTION_ROW_FLOATS;

    // ---- phase 1: poses and W1 -> conv1 --------------------------------------------------------------------------------------------------------
    const long long g = ((long long)(u * a.R + r) * a.Tmax + start0) * D;     // the run's first element of track
    if (S >= F) {
        for (int w = 0; w < nw; ++w)
            egi_stage_exact_t(sm + X_OFF + w * F, XP, a.track, g + (long long)w * S * D, g + ((long long)w * S + F) * D, D, tid, THREADS);
    } else {
        egi_stage_exact_t(sm + X_OFF, XP, a.track, g, g + (long long)((nw - 1) * S + F) * D, D, tid, THREADS);
    }
    stage_weights(sm + W1_OFF, a.w[0], D * 3, C1, tid);
    __syncthreads();
    {
        const bool cut = S >= N1;                       // the windows' conv1 positions are disjoint
        const int cs = S < F ? S : F, count = cut ? nw * N1 : (nw - 1) * S + N1;
        float* a1 = sm + A1_OFF;
        conv_pass<3, 1, 8, C1, true>(sm + X_OFF, XP, sm + W1_OFF, a.b[0], D, count, wave, lane,
                                  [=](int q) { return cut ? (q / N1) * cs + q % N1 : q; },
                                  [=](int q, int co, float s) { a1[co * POS + q] = s; });
    }
    __syncthreads();
    // ---- phase 2: W2 -> conv2 ------------------------------------------------------------------------------------------------------------------
    stage_weights(sm + W2_OFF, a.w[1], C1 * 3, C2, tid);
    __syncthreads();
    {
        const bool cut = S >= N2;
        const int cs = S < N1 ? S : N1, count = cut ? nw * N2 : (nw - 1) * S + N2;
        float* a2 = sm + A2_OFF;
        conv_pass<3, 1, 8, C2, true>(sm + A1_OFF, POS, sm + W2_OFF, a.b[1], C1, count, wave, lane,
                                  [=](int q) { return cut ? (q / N2) * cs + q % N2 : q; },
                                  [=](int q, int co, float s) { a2[co * POS + q] = s; });
    }
    __syncthreads();
    // ---- phase 3: W3, W4 -> conv3, conv4 per batch of windows ------------------------------------------------------------------------------------
    stage_weights(sm + W3_OFF, a.w[2], C2 * 4, C3, tid);
    stage_weights(sm + W4_OFF, a.w[3], C3 * 3, C4, tid);
    if (S < N2 && nw * N3 > (nw - 1) * S + N2 - 3) {    // dense: fewer positions in the run's span than in its windows
        const int count3 = (nw - 1) * S + N2 - 3, count4 = count3 - 4;      // c3[p] reads a2 at p .. p + 3, c4[p] reads c3 at p, p + 2, p + 4
        float *c3 = sm + A3_OFF, *c4 = sm + A2_OFF;
        __syncthreads();                                // the weights are staged
        conv_pass<4, 1, 8, C3, true>(sm + A2_OFF, POS, sm + W3_OFF, a.b[2], C2, count3, wave, lane, [](int q) { return q; },
                                     [=](int q, int co, float s) { c3[co * POS + q] = s; });
        __syncthreads();                                // a2 is consumed: c4 takes its place
        conv_pass<3, 2, 4, C4, false>(c3, POS, sm + W4_OFF, a.b[3], C3, count4, wave, lane, [](int q) { return q; },
                                      [=](int q, int co, float s) { c4[co * POS + q] = s; });
        __syncthreads();
        for (int i = tid; i < nw * EG_MOTION_ROW_FLOATS; i += THREADS) {    // rows[w][co][l] = c4[co][w * S + 2 l], the last read at count4 - 1
            const int w = i / EG_MOTION_ROW_FLOATS, j = i - w * EG_MOTION_ROW_FLOATS, co = j / N4;
            rows[i] = c4[co * POS + w * S + 2 * (j - co * N4)];
        }
        return;
    }
    const int cs2 = S < N2 ? S : N2;
    for (int wb = 0; wb < nw; wb += BATCH) {
        const int nb = nw - wb < BATCH ? nw - wb : BATCH;
        __syncthreads();                                // the weights are staged; the previous batch's a3 is consumed
        float* a3 = sm + A3_OFF;
        conv_pass<4, 1, 8, C3, true>(sm + A2_OFF, POS, sm + W3_OFF, a.b[2], C2, nb * N3, wave, lane,
                                  [=](int q) { const int w = q / N3; return (wb + w) * cs2 + 2 * (q - w * N3); },
                                  [=](int q, int co, float s) { a3[co * P3 + q] = s; });
        __syncthreads();
        float* out = rows + (size_t)wb * EG_MOTION_ROW_FLOATS;
        conv_pass<3, 1, 4, C4, false>(sm + A3_OFF, P3, sm + W4_OFF, a.b[3], C3, nb * N4, wave, lane,
                                   [=](int q) { const int w = q / N4; return w * N3 + (q - w * N4); },
                                   [=](int q, int co, float s) { const int w = q / N4; out[(size_t)w * EG_MOTION_ROW_FLOATS + co * N4 + (q - w * N4)] = s; });
    }
}

}  // namespace

extern "C" int32_t eg_motion_run_windows(int32_t stride) { return stride < 1 ? 0 : run_windows(stride); }

extern "C" int eg_motion_window_rows(const float* track, int32_t U, int32_t R, int32_t Tmax, int32_t D, int32_t window, int32_t S, int32_t tail,
                                     const int32_t* frames, const int32_t* d_frames, const float* w1, const float* b1, const float* w2,
                                     const float* b2, const float* w3, const float* b3, const float* w4, const float* b4, int32_t c0,
                                     int32_t c1, float* rows, void* stream) {
    const char* who = "eg_motion_window_rows";
    const void* ptrs[12] = {track, frames, d_frames, w1, b1, w2, b2, w3, b3, w4, b4, rows};
    const char* names[12] = {"track", "frames", "d_frames", "w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4", "rows"};
    for (int i = 0; i < 12; ++i) EG_REQUIRE(ptrs[i], EG_ERR_BAD_ARG, "%s: null %s", who, names[i]);
    EG_REQUIRE(eg_aligned16(track), EG_ERR_ALIGN, "%s: track not 16-byte aligned", who);
    EG_REQUIRE(eg_aligned16(rows), EG_ERR_ALIGN, "%s: rows not 16-byte aligned", who);
    for (int i = 3; i < 11; ++i)
        EG_REQUIRE((reinterpret_cast<uintptr_t>(ptrs[i]) & 3u) == 0, EG_ERR_ALIGN, "%s: %s not 4-byte aligned", who, names[i]);
    EG_REQUIRE(U >= 1 && U <= MAX_U, EG_ERR_BAD_ARG, "%s: U=%d (1..%d)", who, U, MAX_U);
    EG_REQUIRE(R >= 1 && R <= MAXR, EG_ERR_BAD_ARG, "%s: draws=%d (1..%d)", who, R, MAXR);
    EG_REQUIRE(D >= 1 && D <= MAXD, EG_ERR_BAD_ARG, "%s: pose_dim=%d (1..%d)", who, D, MAXD);
    EG_REQUIRE(window == F, EG_ERR_BAD_ARG, "%s: window=%d (the encoder's out_net is sized for %d frames)", who, window, F);
    EG_REQUIRE(S >= 1, EG_ERR_BAD_ARG, "%s: stride=%d (need >= 1)", who, S);
    EG_REQUIRE(Tmax >= F, EG_ERR_BAD_ARG, "%s: Tmax=%d < window=%d", who, Tmax, F);
    long long clips = 0;
    int maxruns = 0;
    for (int u = 0; u < U; ++u) {
        EG_REQUIRE(frames[u] >= F, EG_ERR_BAD_ARG, "%s: frames[%d]=%d < window=%d (the encoder takes whole windows: no padding, no resampling)",
                   who, u, frames[u], F);
        EG_REQUIRE(frames[u] <= Tmax, EG_ERR_BAD_ARG, "%s: frames[%d]=%d > Tmax=%d", who, u, frames[u], Tmax);
        clips += window_count(frames[u], S, tail);
        const int nr = run_count(frames[u], S, tail);
        maxruns = nr > maxruns ? nr : maxruns;
    }
    const long long N = clips * R;
    EG_REQUIRE(N < (1ll << 31), EG_ERR_UNSUPPORTED, "%s: N=%lld*%d windows: index range (< 2^31)", who, clips, R);
    EG_REQUIRE((double)U * R * (double)Tmax * D < 1099511627776.0, EG_ERR_UNSUPPORTED, "%s: track has %d*%d*%d*%d elements: index range (< 2^40)",
               who, U, R, Tmax, D);
    EG_REQUIRE(c0 >= 0 && c1 <= N && c0 < c1, EG_ERR_BAD_ARG, "%s: clips [%d, %d) (need 0 <= c0 < c1 <= N=%lld)", who, c0, c1, N);
    if (int rc = egi_check_rows(who, U * R, Tmax, nullptr, d_frames, false, R, 1, F, "")) return rc;
    EG_REQUIRE((long long)maxruns * R <= 0x7fffffffll, EG_ERR_UNSUPPORTED, "%s: %lld workgroups per recording: grid range", who,
               (long long)maxruns * R);
    const size_t smem = sizeof(float) * (size_t)LDS_FLOATS;
    if (int rc = eg_ensure_dynamic_lds(reinterpret_cast<const void*>(motion_window_rows_kernel), smem, "motion_window_rows")) return rc;
    MotionArgs a;
    a.track = track; a.meta = d_frames; a.rows = rows;
    a.w[0] = w1; a.w[1] = w2; a.w[2] = w3; a.w[3] = w4;
    a.b[0] = b1; a.b[1] = b2; a.b[2] = b3; a.b[3] = b4;
    a.U = U; a.R = R; a.Tmax = Tmax; a.D = D; a.S = S; a.tail = tail ? 1 : 0; a.maxruns = maxruns; a.c0 = c0; a.c1 = c1;
    hipLaunchKernelGGL(motion_window_rows_kernel, dim3((unsigned)(maxruns * R), (unsigned)U), dim3(THREADS), smem, static_cast<hipStream_t>(stream), a);
    return eg_check_launch("motion_window_rows");
}
