// Emotion recognition of whole tracks (include/emogest.h: eg_emotion_meta, eg_emotion_window_embed, eg_emotion_vote): everything around the
// skeleton emotion classifier for tracks of any and unequal length with R takes each.
//   * emotion_window_embed_kernel: the encoder input of the classifier windows [c0, c1) from the per-pose embedding in packed order plus the
//     positional table -- a window is F consecutive packed rows, so a clip is one contiguous run of F * d_model floats;
//   * emotion_window_kernel: per window the class, per (take, chunk of EG_EMOTION_CHUNK_WINDOWS windows) the fp64 logit sums and the int32
//     counts -> workspace[chunk slot];
//   * emotion_take_kernel: per take the chunk partials in ascending order -> mean_logit, votes, pred (hit, window_hits); workgroup 0 walks
//     all takes in ascending order for the pooled figures.
// Every output element has exactly one owning thread (LDS cells included); plain stores, no atomics, nothing device-scope.  The second vote
// launch reads what the first wrote: the kernel boundary on one stream is the only ordering used.
#include "common.h"

namespace {

constexpr int CH = EG_EMOTION_CHUNK_WINDOWS;
constexpr int MAXC = EG_EMOTION_MAX_CLASSES;
constexpr int MAXR = EG_TAKE_MAX_DRAWS;
constexpr int MAX_U = 65535;                            // blockIdx.y carries the recording
constexpr int TAKE_WAVES = 16;                          // takes of one workgroup of emotion_take_kernel: one wave each
static_assert(CH == EG_WAVE && MAXC == EG_WAVE, "one lane per window of a chunk, one lane per class");

// The chunk slots of recording u start at R * (coff[u] / CH + u): floor((coff + n) / CH) + 1 >= floor(coff / CH) + ceil(n / CH), so the slots of
// consecutive recordings never overlap and the table needs nothing beyond `C | coff`; at most U * R slots stay unused (never written, never read).
__host__ __device__ inline long long slot_base(int coff, int u, int R) { return ((long long)(coff / CH) + u) * R; }
__host__ __device__ inline int window_count(int f, int F, int S, int tail) { return (f - F) / S + 1 + (tail && (f - F) % S != 0 ? 1 : 0); }

// x[(c - c0) * F * Q + i] = emb[row(c) * Q + i] + pos[i] for the F * Q quads i of clip c.  A workgroup takes clips c0 + blockIdx.x,
// + gridDim.x, ...: the search of the clip's recording is workgroup-uniform (scalar loads of the table), the copy is 16 bytes per lane.
__global__ __launch_bounds__(256) void emotion_window_embed_kernel(const f4* __restrict__ emb, const f4* __restrict__ pos, const int* __restrict__ meta,
                                                                   f4* __restrict__ x, int U, int R, int F, int S, int Q, int c0, int c1) {
    const unsigned nq = (unsigned)F * (unsigned)Q;             // quads of one clip (host: < 2^31)
    for (int c = c0 + blockIdx.x; c < c1; c += gridDim.x) {
        int lo = 0, hi = U - 1;                                 // the last recording whose first clip R * coff[u] is <= c
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((long long)R * meta[3 * U + mid] <= (long long)c) lo = mid; else hi = mid - 1;
        }
        const int u = lo, f = meta[u], off = meta[U + u], n = meta[2 * U + u], coff = meta[3 * U + u];
        const int local = (int)((long long)c - (long long)R * coff);      // < R * n
        const int r = local / n, j = local - r * n;
        const int strided = (f - F) / S + 1;                    // windows at 0, S, 2S, ...; the one after them is the tail window
        const int start = j < strided ? j * S : f - F;
        const f4* src = emb + ((size_t)R * off + (size_t)r * f + (size_t)start) * Q;
        f4* dst = x + (size_t)(c - c0) * nq;
        for (unsigned i = threadIdx.x; i < nq; i += 256u) {
            const f4 a = src[i], p = pos[i];
            f4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = a[e] + p[e];
            dst[i] = v;
        }
    }
}

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// One wave per (take, chunk): blockIdx.y = u, blockIdx.x = r * maxch + chunk.  Lane w classifies window w of the chunk; then lane c adds
// the chunk's valid windows' logit c in ascending window order (fp32 widened) and counts the windows of class c.
__global__ __launch_bounds__(64) void emotion_window_kernel(const float* __restrict__ logits, const int* __restrict__ cnt, double* __restrict__ dsum,
                                                            int* __restrict__ icnt, int* __restrict__ wclass, int U, int R, int C, int maxch) {
    const int u = blockIdx.y;
    const int n = cnt[u], coff = cnt[U + u];
    const int r = blockIdx.x / maxch, ch = blockIdx.x - r * maxch;
    const int nch = (n + CH - 1) / CH;
    if (ch >= nch) return;                                      // workgroup-uniform: fewer chunks than the grid's longest take
    const int w0 = ch * CH;
    const int nw = n - w0 < CH ? n - w0 : CH;
    const size_t first = (size_t)((long long)R * coff + (long long)r * n + w0);      // the chunk's first clip
    const size_t slot = (size_t)(slot_base(coff, u, R) + (long long)r * nch + ch);
    const int lane = threadIdx.x;
    __shared__ int cls[CH];
    int k = -1;
    if (lane < nw) {
        const float* l = logits + (first + lane) * C;
        float best = l[0];
        bool ok = finite_f32(best);
        int bi = 0;
        for (int c = 1; c < C; ++c) {
            const float v = l[c];
            ok = ok && finite_f32(v);
            if (v > best) { best = v; bi = c; }                 // strict: the lowest index among equal maxima
        }
        k = ok ? bi : -1;
        wclass[first + lane] = k;
    }
    cls[lane] = k;
    __syncthreads();
    if (lane < C) {
        const float* l = logits + first * C + lane;
        double s = 0.0;
        int votes = 0;
        for (int w = 0; w < nw; ++w) {
            const int kw = cls[w];
            if (kw >= 0) {
                s += (double)l[(size_t)w * C];
                votes += kw == lane ? 1 : 0;
            }
        }
        dsum[slot * C + lane] = s;
        icnt[slot * (C + 1) + lane] = votes;
    }
    if (lane == 0) {
        int inv = 0;
        for (int w = 0; w < nw; ++w) inv += cls[w] < 0 ? 1 : 0;
        icnt[slot * (C + 1) + C] = inv;
    }
}

struct TakeResult { int votes; double mean; int pred; int invalid; };      // votes / mean: this lane's class; pred / invalid: the take's

// The whole wave calls this for take (u, r); lane c < C owns class c.  The same function serves the per-take workgroups and the pooled one,
// so both see the same pred.
__device__ __forceinline__ TakeResult take_reduce(const int* __restrict__ cnt, const double* __restrict__ dsum, const int* __restrict__ icnt,
                                                  int U, int R, int C, int u, int r, int lane) {
    const int n = cnt[u], coff = cnt[U + u];
    const int nch = (n + CH - 1) / CH;
    const size_t slot0 = (size_t)(slot_base(coff, u, R) + (long long)r * nch);
    double s = 0.0;
    int votes = -1, inv = 0;
    if (lane < C) {
        votes = 0;
        for (int c = 0; c < nch; ++c) {                         // ascending chunks
            s += dsum[(slot0 + c) * C + lane];
            votes += icnt[(slot0 + c) * (C + 1) + lane];
        }
    }
    for (int c = 0; c < nch; ++c) inv += icnt[(slot0 + c) * (C + 1) + C];
    const int count = n - inv;
    TakeResult res;
    res.votes = votes;
    res.invalid = inv;
    res.mean = count > 0 ? s / (double)count : __longlong_as_double(0x7ff8000000000000ll);
    // most votes; among them the larger mean; still tied, the lowest class: a total order, so the butterfly leaves one winner in every lane
    int bv = votes, bi = lane;
    double bm = res.mean;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int ov = __shfl_xor(bv, o, 64), oi = __shfl_xor(bi, o, 64);
        const double om = __shfl_xor(bm, o, 64);
        const bool take = ov > bv || (ov == bv && (om > bm || (om == bm && oi < bi)));
        if (take) { bv = ov; bm = om; bi = oi; }
    }
    res.pred = count > 0 ? bi : -1;
    return res;
}

// Workgroups 1 ..: TAKE_WAVES takes each, one wave per take.  Workgroup 0: the pooled figures -- it walks all takes in ascending order,
// TAKE_WAVES at a time, recomputing each take's result from the workspace (it cannot read what the other workgroups of this launch write);
// every cell of the two matrices in LDS has one owning thread: column c = tid % 64, rows y with y % TAKE_WAVES == tid / 64.
__global__ __launch_bounds__(64 * TAKE_WAVES) void emotion_take_kernel(const int* __restrict__ cnt, const double* __restrict__ dsum,
                                                                      const int* __restrict__ icnt, const int* __restrict__ labels,
                                                                      int* __restrict__ votes, int* __restrict__ invalid, double* __restrict__ mean_logit,
                                                                      int* __restrict__ pred, int* __restrict__ hit, int* __restrict__ window_hits,
                                                                      double* __restrict__ accuracy, double* __restrict__ window_accuracy,
                                                                      int* __restrict__ confusion, int* __restrict__ window_confusion,
                                                                      int* __restrict__ unscored, int U, int R, int C, long long windows) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int takes = U * R;                                    // host: < 2^31
    if (blockIdx.x > 0) {
        const int t = (blockIdx.x - 1) * TAKE_WAVES + wave;
        if (t >= takes) return;                                 // wave-uniform; no barrier below
        const TakeResult res = take_reduce(cnt, dsum, icnt, U, R, C, t / R, t % R, lane);
        if (lane < C) {
            votes[(size_t)t * C + lane] = res.votes;
            mean_logit[(size_t)t * C + lane] = res.mean;
        }
        int y = labels ? labels[t] : -1;
        if (y < 0 || y >= C) y = -1;                            // a label outside [0, C) is never used as an index
        const int vy = __shfl(res.votes, y < 0 ? 0 : y, 64);
        if (lane == 0) {
            invalid[t] = res.invalid;
            pred[t] = res.pred;
            if (labels) {
                hit[t] = y >= 0 && res.pred == y ? 1 : 0;
                window_hits[t] = y >= 0 ? vy : 0;
            }
        }
        return;
    }
    __shared__ int conf[MAXC * MAXC], wconf[MAXC * MAXC];
    __shared__ int tvotes[TAKE_WAVES][MAXC], tpred[TAKE_WAVES], ty[TAKE_WAVES];
    for (int i = tid; i < C * C; i += 64 * TAKE_WAVES) { conf[i] = 0; wconf[i] = 0; }
    long long hits = 0, whits = 0;                              // thread 0's
    int unsc = 0;
    for (int t0 = 0; t0 < takes; t0 += TAKE_WAVES) {
        const int t = t0 + wave;
        __syncthreads();                                        // the previous tile is consumed (and the matrices are cleared)
        if (t < takes) {
            const TakeResult res = take_reduce(cnt, dsum, icnt, U, R, C, t / R, t % R, lane);
            tvotes[wave][lane] = lane < C ? res.votes : 0;
            if (lane == 0) {
                int y = labels ? labels[t] : -1;
                tpred[wave] = res.pred;
                ty[wave] = y < 0 || y >= C ? -1 : y;
            }
        } else if (lane == 0) {
            ty[wave] = -2;                                      // no take
        }
        __syncthreads();
        if (labels && lane < C) {
            for (int k = 0; k < TAKE_WAVES; ++k) {              // ascending takes
                const int y = ty[k];
                if (y >= 0 && (y % TAKE_WAVES) == wave) {
                    wconf[y * C + lane] += tvotes[k][lane];
                    if (tpred[k] == lane) conf[y * C + lane] += 1;
                }
            }
        }
        if (tid == 0) {
            for (int k = 0; k < TAKE_WAVES; ++k) {
                const int y = ty[k], p = tpred[k];
                if (y == -2) continue;
                if (p < 0 || (labels && y < 0)) { ++unsc; continue; }
                if (labels) {
                    hits += p == y ? 1 : 0;
                    whits += tvotes[k][y];
                }
            }
        }
    }
    __syncthreads();
    if (labels) {
        for (int i = tid; i < C * C; i += 64 * TAKE_WAVES) { confusion[i] = conf[i]; window_confusion[i] = wconf[i]; }
    }
    if (tid == 0) {
        *unscored = unsc;
        if (labels) {
            *accuracy = 100.0 * (double)hits / (double)takes;
            *window_accuracy = 100.0 * (double)whits / (double)windows;
        }
    }
}

// Shared host checks of a frames vector against the window: returns sum(C_u) or -1 (error set, `who` first); sum(frames) through *rows.
long long check_windows(const char* who, const int32_t* frames, int U, int F, int S, int tail, long long* rows) {
    if (!frames) { eg_set_error("%s: null frames", who); return -1; }
    if (U < 1 || U > MAX_U) { eg_set_error("%s: U=%d (1..%d)", who, U, MAX_U); return -1; }
    if (F < 1) { eg_set_error("%s: window=%d (need >= 1)", who, F); return -1; }
    if (S < 1) { eg_set_error("%s: stride=%d (need >= 1)", who, S); return -1; }
    long long sum = 0, clips = 0;
    for (int u = 0; u < U; ++u) {
        if (frames[u] < F) {
            eg_set_error("%s: frames[%d]=%d < window=%d (the classifier takes whole windows: no padding, no resampling)", who, u, frames[u], F);
            return -1;
        }
        sum += frames[u];
        clips += window_count(frames[u], F, S, tail);
    }
    if (sum >= (1ll << 31)) { eg_set_error("%s: sum(frames)=%lld: index range (< 2^31)", who, sum); return -1; }
    if (rows) *rows = sum;
    return clips;
}

// Host checks of a window-count vector: returns sum(counts) or -1.
long long check_counts(const char* who, const int32_t* counts, int U, int R, int C) {
    if (!counts) { eg_set_error("%s: null counts", who); return -1; }
    if (U < 1 || U > MAX_U) { eg_set_error("%s: U=%d (1..%d)", who, U, MAX_U); return -1; }
    if (R < 1 || R > MAXR) { eg_set_error("%s: draws=%d (1..%d)", who, R, MAXR); return -1; }
    if (C < 2 || C > MAXC) { eg_set_error("%s: classes=%d (2..%d)", who, C, MAXC); return -1; }
    long long sum = 0;
    for (int u = 0; u < U; ++u) {
        if (counts[u] < 1) { eg_set_error("%s: counts[%d]=%d (need >= 1)", who, u, counts[u]); return -1; }
        sum += counts[u];
    }
    if (sum * R >= (1ll << 31)) { eg_set_error("%s: N=%lld*%d windows: index range (< 2^31)", who, sum, R); return -1; }
    return sum;
}

long long vote_bytes(long long sum, int U, int R, int C) {
    const long long slots = (sum / CH + U) * R;
    return eg_round_up(slots * C * (long long)sizeof(double), 16) + eg_round_up(slots * (C + 1) * (long long)sizeof(int32_t), 16);
}

}  // namespace

extern "C" int64_t eg_emotion_meta_ints(int32_t recordings) { return recordings < 1 || recordings > MAX_U ? 0 : 4 * (int64_t)recordings; }

extern "C" int64_t eg_emotion_meta(const int32_t* frames, int32_t recordings, int32_t window, int32_t stride, int32_t tail, int32_t* meta) {
    const char* who = "eg_emotion_meta";
    const long long clips = check_windows(who, frames, recordings, window, stride, tail, nullptr);
    if (clips < 0) return 0;
    if (!meta) { eg_set_error("%s: null meta", who); return 0; }
    const int U = recordings;                                   // C_u <= frames[u]: sum(C) is in range with sum(frames)
    int32_t off = 0, coff = 0;
    for (int u = 0; u < U; ++u) {
        const int32_t n = window_count(frames[u], window, stride, tail);
        meta[u] = frames[u];
        meta[U + u] = off;
        meta[2 * U + u] = n;
        meta[3 * U + u] = coff;
        off += frames[u];
        coff += n;
    }
    return clips;
}

extern "C" int eg_emotion_window_embed(const float* emb, const float* pos, int32_t U, int32_t R, int32_t F, int32_t S, int32_t tail,
                                       int32_t d_model, const int32_t* frames, const int32_t* d_meta, int32_t c0, int32_t c1, float* x,
                                       void* stream) {
    const char* who = "eg_emotion_window_embed";
    const void* ptrs[4] = {emb, pos, d_meta, x};
    const char* names[4] = {"emb", "pos", "d_meta", "x"};
    for (int i = 0; i < 4; ++i) EG_REQUIRE(ptrs[i], EG_ERR_BAD_ARG, "%s: null %s", who, names[i]);
    for (int i = 0; i < 4; ++i) EG_REQUIRE(i == 2 || eg_aligned16(ptrs[i]), EG_ERR_ALIGN, "%s: %s not 16-byte aligned", who, names[i]);
    EG_REQUIRE(R >= 1 && R <= MAXR, EG_ERR_BAD_ARG, "%s: draws=%d (1..%d)", who, R, MAXR);
    EG_REQUIRE(d_model >= 4 && d_model % 4 == 0, EG_ERR_BAD_ARG, "%s: d_model=%d (a multiple of 4, >= 4: 16-byte loads and stores)", who, d_model);
    long long rows = 0;
    const long long clips = check_windows(who, frames, U, F, S, tail, &rows);
    if (clips < 0) return EG_ERR_BAD_ARG;
    const long long N = clips * R;
    EG_REQUIRE(N < (1ll << 31), EG_ERR_UNSUPPORTED, "%s: N=%lld*%d windows: index range (< 2^31)", who, clips, R);
    EG_REQUIRE((long long)F * (d_model / 4) < (1ll << 31), EG_ERR_UNSUPPORTED, "%s: window*d_model=%d*%d: index range", who, F, d_model);
    EG_REQUIRE((double)R * (double)rows * (double)d_model < 1099511627776.0, EG_ERR_UNSUPPORTED, "%s: rows*d_model=%lld*%d: index range (< 2^40)",
               who, R * rows, d_model);
    EG_REQUIRE(c0 >= 0 && c1 <= N && c0 < c1, EG_ERR_BAD_ARG, "%s: clips [%d, %d) (need 0 <= c0 < c1 <= N=%lld)", who, c0, c1, N);
    const int n = c1 - c0;
    const int gx = n < 2048 ? n : 2048;                         // 8 workgroups per CU, the rest by the grid stride
    hipLaunchKernelGGL(emotion_window_embed_kernel, dim3((unsigned)gx), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const f4*>(emb), reinterpret_cast<const f4*>(pos), d_meta, reinterpret_cast<f4*>(x), U, R, F, S,
                       d_model / 4, c0, c1);
    return eg_check_launch("emotion_window_embed");
}

extern "C" int64_t eg_emotion_vote_workspace_bytes(const int32_t* counts, int32_t recordings, int32_t draws, int32_t classes) {
    const long long sum = check_counts("eg_emotion_vote_workspace_bytes", counts, recordings, draws, classes);
    return sum < 0 ? 0 : vote_bytes(sum, recordings, draws, classes);
}

extern "C" int eg_emotion_vote(const float* logits, int32_t U, int32_t R, int32_t C, const int32_t* counts, const int32_t* d_counts,
                               const int32_t* d_labels, void* workspace, int64_t workspace_bytes, int32_t* window_class, int32_t* votes,
                               int32_t* invalid, double* mean_logit, int32_t* pred, int32_t* hit, int32_t* window_hits, double* accuracy,
                               double* window_accuracy, int32_t* confusion, int32_t* window_confusion, int32_t* unscored, void* stream) {
    const char* who = "eg_emotion_vote";
    const void* ptrs[9] = {logits, d_counts, workspace, window_class, votes, invalid, mean_logit, pred, unscored};
    const char* names[9] = {"logits", "d_counts", "workspace", "window_class", "votes", "invalid", "mean_logit", "pred", "unscored"};
    for (int i = 0; i < 9; ++i) EG_REQUIRE(ptrs[i], EG_ERR_BAD_ARG, "%s: null %s", who, names[i]);
    if (d_labels) {
        const void* lp[6] = {hit, window_hits, accuracy, window_accuracy, confusion, window_confusion};
        const char* ln[6] = {"hit", "window_hits", "accuracy", "window_accuracy", "confusion", "window_confusion"};
        for (int i = 0; i < 6; ++i) EG_REQUIRE(lp[i], EG_ERR_BAD_ARG, "%s: null %s (needed with d_labels)", who, ln[i]);
    }
    EG_REQUIRE(eg_aligned16(workspace), EG_ERR_ALIGN, "%s: workspace not 16-byte aligned", who);
    const void* dp[3] = {mean_logit, accuracy, window_accuracy};
    const char* dn[3] = {"mean_logit", "accuracy", "window_accuracy"};
    for (int i = 0; i < 3; ++i)
        EG_REQUIRE((reinterpret_cast<uintptr_t>(dp[i]) & 7u) == 0, EG_ERR_ALIGN, "%s: %s not 8-byte aligned", who, dn[i]);
    EG_REQUIRE((reinterpret_cast<uintptr_t>(logits) & 3u) == 0, EG_ERR_ALIGN, "%s: logits not 4-byte aligned", who);
    const long long sum = check_counts(who, counts, U, R, C);
    if (sum < 0) return EG_ERR_BAD_ARG;
    const long long need = vote_bytes(sum, U, R, C);
    EG_REQUIRE(workspace_bytes >= need, EG_ERR_WORKSPACE, "%s: workspace too small (%lld < %lld bytes)", who, (long long)workspace_bytes, need);
    int maxn = 0;
    for (int u = 0; u < U; ++u) maxn = counts[u] > maxn ? counts[u] : maxn;
    const int maxch = (maxn + CH - 1) / CH;
    EG_REQUIRE((long long)maxch * R <= 0x7fffffffll, EG_ERR_UNSUPPORTED, "%s: %lld workgroups per recording: grid range", who, (long long)maxch * R);
    const long long slots = (sum / CH + U) * R;
    double* dsum = static_cast<double*>(workspace);
    int* icnt = reinterpret_cast<int*>(static_cast<char*>(workspace) + eg_round_up(slots * C * (long long)sizeof(double), 16));
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(emotion_window_kernel, dim3((unsigned)(maxch * R), (unsigned)U), dim3(64), 0, st, logits, d_counts, dsum, icnt,
                       window_class, U, R, C, maxch);
    int rc = eg_check_launch("emotion_window");
    if (rc != EG_OK) return rc;
    const long long takes = (long long)U * R;
    const unsigned gx = 1u + (unsigned)((takes + TAKE_WAVES - 1) / TAKE_WAVES);
    hipLaunchKernelGGL(emotion_take_kernel, dim3(gx), dim3(64 * TAKE_WAVES), 0, st, d_counts, dsum, icnt, d_labels, votes, invalid, mean_logit,
                       pred, hit, window_hits, accuracy, window_accuracy, confusion, window_confusion, unscored, U, R, C, sum * R);
    return eg_check_launch("emotion_take");
}
