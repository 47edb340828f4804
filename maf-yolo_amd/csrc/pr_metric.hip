// In-process precision / recall / mAP of an evaluation on the device — the `do_pr_metric` path of Evaler.predict_model
// (yolov6/core/evaler.py:195-268) with yolov6/utils/metrics.py process_batch, ConfusionMatrix.process_batch, ap_per_class and compute_ap.
// The rules are those of tests/pr_metric_ref.py: masks and confusion counts bit for bit, curves in fp64 without FMA contraction (this
// file is compiled with -ffp-contract=off).
//
//   maf_pr_match   one launch per batch, one workgroup per image: labels gathered into LDS (target order kept), labels and detections
//                  taken to native space (scale_coords.h), per detection its best same-class label and the uint16 mask of thresholds
//                  it is correct at, the optional confusion matrix, per-class label / prediction counts, and one record per detection
//                  (sort key, mask) appended at the dataset-wide position offs[0] + (rows of earlier images).
//   maf_pr_curves  once per evaluation, after the records are sorted by key (class, conf descending; a stable sort keeps image order,
//                  then NMS row order): class offsets (a scan of the counts), the tp / fp cumulative sums, recall, precision and the
//                  precision envelope of each (class, threshold) segment, np.interp at the 1000 + 101 grid points, the trapezoid AP;
//                  then the summary.  Three stream-ordered launches.
#include "maf_common.h"
#include "block_scan.h"
#include "scale_coords.h"

namespace {

constexpr int MATCH_THREADS = 256;
constexpr int CURVE_THREADS = 1024;

struct MatchArgs {
    const float* rows; const int* count; const float* targets; const float* img; const float* iouv;
    const int64_t* offs_in; int64_t* offs_out; int64_t* keys; uint16_t* masks; int* state;
    int64_t capacity;
    int B, max_det, n_targets, H, W, niou, nc, flags;
    float cm_conf, cm_iou;
};

__device__ __forceinline__ bool valid_cls(float c, int nc) { return c >= 0.f && c < (float)nc && c == floorf(c); }

// fp32 box_iou of one (label, detection) pair: inter / (area1 + area2 - inter)
__device__ __forceinline__ float pair_iou(const float* l, float la, float x1, float y1, float x2, float y2, float da) {
    const float w = fmaxf(fminf(l[2], x2) - fmaxf(l[0], x1), 0.f);
    const float h = fmaxf(fminf(l[3], y2) - fmaxf(l[1], y1), 0.f);
    const float inter = w * h;
    return inter / ((la + da) - inter);
}

// order-preserving uint32 of an fp32 (ascending), complemented: ascending keys = descending confidence
__device__ __forceinline__ uint32_t desc_bits(float f) {
    uint32_t u = __float_as_uint(f + 0.f);                 // -0 -> +0: equal confidences must tie
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}

__global__ __launch_bounds__(MATCH_THREADS) void pr_match_kernel(const MatchArgs a) {
    __shared__ float lbox[MAF_PR_MAX_LABELS][4];
    __shared__ float larea[MAF_PR_MAX_LABELS];
    __shared__ int lcls[MAF_PR_MAX_LABELS];
    __shared__ int lmatch[MAF_PR_MAX_LABELS];
    __shared__ int dbest[MAF_PR_MAX_DET];
    __shared__ float diou[MAF_PR_MAX_DET];
    __shared__ float iouv[16];
    __shared__ int wave_n[MATCH_THREADS / 64];
    __shared__ int s_base, s_any, s_match;
    int* err = a.state;
    int* any_correct = a.state + 1;
    int* nt = a.state + 2;
    int* npc = nt + a.nc;
    int* matrix = npc + a.nc;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        int base = 0;
        for (int i = 0; i < b; ++i) base += min(max(a.count[i], 0), a.max_det);
        s_base = base; s_any = 0; s_match = 0;
    }
    if (tid < a.niou) iouv[tid] = a.iouv[tid];
    __syncthreads();
    const int n = min(max(a.count[b], 0), a.max_det);
    const int64_t off = a.offs_in[0] + s_base;
    if (b == a.B - 1 && tid == 0) a.offs_out[0] = off + n;
    const bool xyxy = a.flags & MAF_PR_LABELS_XYXY;
    const float* par = a.img + b * 6;

    // 1. this image's labels, in target order (an ordered compaction of the rows whose image index is b)
    int nl = 0;
    for (int t0 = 0; t0 < a.n_targets; t0 += MATCH_THREADS) {
        const int t = t0 + tid;
        const bool mine = t < a.n_targets && a.targets[(size_t)t * 6] == (float)b;
        const uint64_t bal = __ballot(mine);
        if (lane == 0) wave_n[wave] = __popcll(bal);
        __syncthreads();
        int pos = nl, total = 0;
        for (int w = 0; w < MATCH_THREADS / 64; ++w) {
            if (w < wave) pos += wave_n[w];
            total += wave_n[w];
        }
        pos += __popcll(bal & ((1ull << lane) - 1ull));
        if (mine) {
            const float* r = a.targets + (size_t)t * 6;
            const float c = r[1];
            if (!valid_cls(c, a.nc)) atomicOr(err, MAF_PR_ERR_CLASS);
            else atomicAdd(&nt[(int)c], 1);
            if (pos < MAF_PR_MAX_LABELS) {
                float x1, y1, x2, y2;
                if (xyxy) {
                    x1 = r[2]; y1 = r[3]; x2 = r[4]; y2 = r[5];
                } else {                                   // xywh2xyxy, * letterboxed W / H, scale_coords
                    x1 = r[2] - r[4] / 2.f; y1 = r[3] - r[5] / 2.f; x2 = r[2] + r[4] / 2.f; y2 = r[3] + r[5] / 2.f;
                    x1 *= (float)a.W; x2 *= (float)a.W; y1 *= (float)a.H; y2 *= (float)a.H;
                    maf_scale_box(x1, y1, x2, y2, par);
                }
                lbox[pos][0] = x1; lbox[pos][1] = y1; lbox[pos][2] = x2; lbox[pos][3] = y2;
                larea[pos] = (x2 - x1) * (y2 - y1);
                lcls[pos] = valid_cls(c, a.nc) ? (int)c : -2;   // matches no detection (the error flag is set)
                lmatch[pos] = -1;
            }
        }
        nl += total;
        __syncthreads();
    }
    if (nl > MAF_PR_MAX_LABELS) {
        if (tid == 0) atomicOr(err, MAF_PR_ERR_LABELS);
        nl = MAF_PR_MAX_LABELS;
    }
    if (n > 0 && off + n > a.capacity) {                   // never with the host's bound; keeps every store inside the buffer
        if (tid == 0) atomicOr(err, MAF_PR_ERR_CAPACITY);
        return;
    }

    // 2. per detection: native-space box, best same-class label (equal IoU: the lower label index)
    for (int k = tid; k < n; k += MATCH_THREADS) {
        const float* r = a.rows + ((size_t)b * a.max_det + k) * 6;
        float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
        if (!xyxy) maf_scale_box(x1, y1, x2, y2, par);
        const float da = (x2 - x1) * (y2 - y1);
        const float c = r[5];
        int dc = -1;
        if (!valid_cls(c, a.nc)) atomicOr(err, MAF_PR_ERR_CLASS);
        else { dc = (int)c; atomicAdd(&npc[dc], 1); }
        int bj = -1;
        float best = -1.f;
        for (int j = 0; j < nl; ++j) {
            if (lcls[j] != dc) continue;
            const float iou = pair_iou(lbox[j], larea[j], x1, y1, x2, y2, da);
            if (iou > best) { best = iou; bj = j; }
        }
        dbest[k] = bj; diou[k] = best;
    }
    __syncthreads();

    // 3. the correct mask: at threshold t, k is correct iff its best IoU >= t and no lower-index detection with the same best label
    //    reaches t; then the record (key, mask)
    for (int k = tid; k < n; k += MATCH_THREADS) {
        const int bj = dbest[k];
        uint32_t m = 0;
        if (bj >= 0) {
            float prev = -1.f;
            for (int j = 0; j < k; ++j)
                if (dbest[j] == bj) prev = fmaxf(prev, diou[j]);
            for (int t = 0; t < a.niou; ++t)
                if (diou[k] >= iouv[t] && !(prev >= iouv[t])) m |= 1u << t;
        }
        if (m) s_any = 1;
        const float* r = a.rows + ((size_t)b * a.max_det + k) * 6;
        const float c = r[5];
        const int64_t cls = valid_cls(c, a.nc) ? (int64_t)c : (int64_t)a.nc;
        a.keys[off + k] = (cls << 32) | (int64_t)desc_bits(r[4]);
        a.masks[off + k] = (uint16_t)m;
    }
    __syncthreads();
    if (tid == 0 && s_any) atomicOr(any_correct, 1);

    // 4. ConfusionMatrix.process_batch (images with detections and labels): detections with conf > cm_conf, class-agnostic iou > cm_iou,
    //    per detection its best label (lower label index on ties), per label its best detection among those (lower index on ties)
    if (!(a.flags & MAF_PR_CONFUSION) || n == 0 || nl == 0) return;
    const int nc1 = a.nc + 1;
    for (int k = tid; k < n; k += MATCH_THREADS) {
        const float* r = a.rows + ((size_t)b * a.max_det + k) * 6;
        int bj = -1;
        float best = -1.f;
        if (r[4] > a.cm_conf) {
            float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
            if (!xyxy) maf_scale_box(x1, y1, x2, y2, par);
            const float da = (x2 - x1) * (y2 - y1);
            for (int j = 0; j < nl; ++j) {
                const float iou = pair_iou(lbox[j], larea[j], x1, y1, x2, y2, da);
                if (iou > a.cm_iou && iou > best) { best = iou; bj = j; }
            }
        }
        dbest[k] = bj; diou[k] = best;
    }
    __syncthreads();
    for (int l = tid; l < nl; l += MATCH_THREADS) {
        int bk = -1;
        float best = -1.f;
        for (int k = 0; k < n; ++k)
            if (dbest[k] == l && diou[k] > best) { best = diou[k]; bk = k; }
        lmatch[l] = bk;
        if (bk >= 0) s_match = 1;
        const int gc = lcls[l];
        if (gc < 0) continue;
        if (bk >= 0) {
            const int dc = (int)a.rows[((size_t)b * a.max_det + bk) * 6 + 5];
            if (dc >= 0 && dc < a.nc) atomicAdd(&matrix[dc * nc1 + gc], 1);
        } else {
            atomicAdd(&matrix[a.nc * nc1 + gc], 1);
        }
    }
    __syncthreads();
    if (!s_match) return;
    for (int k = tid; k < n; k += MATCH_THREADS) {
        const float* r = a.rows + ((size_t)b * a.max_det + k) * 6;
        if (!(r[4] > a.cm_conf)) continue;                 // not in the filtered list
        const int bj = dbest[k];
        if (bj >= 0 && lmatch[bj] == k) continue;
        const int dc = (int)r[5];
        if (dc >= 0 && dc < a.nc) atomicAdd(&matrix[dc * nc1 + a.nc], 1);
    }
}

// ---- curves -------------------------------------------------------------------------------------------------------------------

struct CurveArgs {
    const int64_t* skeys; const int64_t* perm; const uint16_t* masks; const int* state;
    int64_t* coff; int* tpc; double* env; double* out;
    int64_t capacity;
    int nc, niou;
};

__global__ __launch_bounds__(64) void pr_offsets_kernel(const CurveArgs a) {
    if (threadIdx.x != 0) return;
    const int* npc = a.state + 2 + a.nc;
    int64_t s = 0;
    for (int c = 0; c < a.nc; ++c) { a.coff[c] = s; s += npc[c]; }
    a.coff[a.nc] = s;
}

// np.interp(x, xp, fp, left, right) over a monotone virtual array: j = the last index with xp[j] <= x
template <class XP, class FP>
__device__ double np_interp(double x, int64_t len, XP xp, FP fp, double left, double right) {
    if (x > xp(len - 1)) return right;
    if (x < xp(0)) return left;
    int64_t lo = 0, hi = len;                              // upper bound
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (x >= xp(mid)) lo = mid + 1; else hi = mid;
    }
    const int64_t j = lo - 1;
    if (j == len - 1) return fp(j);
    const double xj = xp(j);
    if (xj == x) return fp(j);
    const double fj = fp(j);
    const double slope = (fp(j + 1) - fj) / (xp(j + 1) - xj);
    return slope * (x - xj) + fj;
}

// numpy's pairwise add.reduce for n <= 128 (8 partial sums), sequential beyond
__device__ double np_sum(const double* v, int n, int stride) {
    if (n < 8 || n > 128) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += v[(size_t)i * stride];
        return s;
    }
    double r[8];
    for (int i = 0; i < 8; ++i) r[i] = v[(size_t)i * stride];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int q = 0; q < 8; ++q) r[q] += v[(size_t)(i + q) * stride];
    double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) s += v[(size_t)i * stride];
    return s;
}

__device__ __forceinline__ double px_at(int k) { return k == 999 ? 1.0 : (double)k * (1.0 / 999.0); }
__device__ __forceinline__ double x101_at(int k) { return k == 100 ? 1.0 : (double)k * (1.0 / 100.0); }

// one workgroup per (class, threshold): the segment of class c in the sorted records
__global__ __launch_bounds__(CURVE_THREADS) void pr_curves_kernel(const CurveArgs a) {
    __shared__ int shi[CURVE_THREADS];
    __shared__ double shd[CURVE_THREADS];
    __shared__ double yap[101];
    const int c = blockIdx.x, j = blockIdx.y, tid = threadIdx.x;
    const int nc = a.nc, niou = a.niou;
    const int* nt = a.state + 2;
    const int64_t s = a.coff[c], L = a.coff[c + 1] - s;
    const int nl = nt[c];
    double* P = a.out + MAF_PR_HEADER;
    double* R = P + (size_t)nc * 1000;
    double* F1 = R + (size_t)nc * 1000;
    double* PY = F1 + (size_t)nc * 1000;
    double* AP = PY + (size_t)nc * 1000;
    if (nl == 0 || L == 0) {
        if (j == 0)
            for (int k = tid; k < 1000; k += CURVE_THREADS) {
                P[(size_t)c * 1000 + k] = 0.0; R[(size_t)c * 1000 + k] = 0.0; F1[(size_t)c * 1000 + k] = 0.0; PY[(size_t)c * 1000 + k] = 0.0;
            }
        if (tid == 0) AP[(size_t)c * niou + j] = 0.0;
        return;
    }
    int* T = a.tpc + (size_t)j * a.capacity + s;
    double* E = a.env + (size_t)j * a.capacity + s;
    const int64_t chunk = (L + CURVE_THREADS - 1) / CURVE_THREADS;
    const int64_t i0 = min(L, chunk * tid), i1 = min(L, i0 + chunk);
    // tp count of this thread's chunk -> its starting cumulative sum
    int cnt = 0;
    for (int64_t i = i0; i < i1; ++i) cnt += (a.masks[a.perm[s + i]] >> j) & 1;
    int tpc = block_excl_sum<CURVE_THREADS>(cnt, shi);
    double cmax = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
        tpc += (a.masks[a.perm[s + i]] >> j) & 1;
        T[i] = tpc;
        cmax = fmax(cmax, (double)tpc / (double)(i + 1));
    }
    // precision envelope: suffix maximum (the trailing 0 of compute_ap never wins: precision >= 0)
    double run = block_suffix_max_after<CURVE_THREADS>(cmax, shd);
    for (int64_t i = i1 - 1; i >= i0; --i) {
        run = fmax(run, (double)T[i] / (double)(i + 1));
        E[i] = run;
    }
    __syncthreads();
    const double nld = (double)nl + 1e-16;
    // compute_ap's arrays: mrec = [0, recall, recall[-1] + 0.01], mpre = envelope of [1, precision, 0]
    auto mrec = [&](int64_t q) -> double {
        if (q == 0) return 0.0;
        if (q <= L) return (double)T[q - 1] / nld;
        return (double)T[L - 1] / nld + 0.01;
    };
    auto mpre = [&](int64_t q) -> double {
        if (q == 0) return 1.0;
        if (q <= L) return E[q - 1];
        return 0.0;
    };
    for (int k = tid; k < 101; k += CURVE_THREADS) yap[k] = np_interp(x101_at(k), L + 2, mrec, mpre, mpre(0), mpre(L + 1));
    __syncthreads();
    if (tid == 0) {
        double d[100];
        for (int k = 0; k < 100; ++k) d[k] = (x101_at(k + 1) - x101_at(k)) * (yap[k + 1] + yap[k]) / 2.0;
        AP[(size_t)c * niou + j] = np_sum(d, 100, 1);
    }
    if (j != 0) return;
    // threshold 0: r, p at -px over -conf (left 0 / 1), py = the envelope on px, f1
    auto negconf = [&](int64_t q) -> double {
        const uint32_t u = ~(uint32_t)(a.skeys[s + q] & 0xffffffffll);
        const uint32_t bits = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
        return -(double)__uint_as_float(bits);
    };
    auto recall = [&](int64_t q) -> double { return (double)T[q] / nld; };
    auto precision = [&](int64_t q) -> double { return (double)T[q] / (double)(q + 1); };
    for (int k = tid; k < 1000; k += CURVE_THREADS) {
        const double x = px_at(k);
        const double r = np_interp(-x, L, negconf, recall, 0.0, recall(L - 1));
        const double p = np_interp(-x, L, negconf, precision, 1.0, precision(L - 1));
        R[(size_t)c * 1000 + k] = r;
        P[(size_t)c * 1000 + k] = p;
        F1[(size_t)c * 1000 + k] = 2.0 * p * r / (p + r + 1e-16);
        PY[(size_t)c * 1000 + k] = np_interp(x, L + 2, mrec, mpre, mpre(0), mpre(L + 1));
    }
}

// the summary of Evaler.predict_model (:240-268) and the integer state copied into the output, one workgroup
__global__ __launch_bounds__(CURVE_THREADS) void pr_summary_kernel(const CurveArgs a) {
    __shared__ double mean[1000];
    __shared__ double col[MAF_PR_MAX_CLASSES];
    const int tid = threadIdx.x, nc = a.nc, niou = a.niou;
    const int* nt = a.state + 2;
    const int* cm = nt + 2 * nc;
    double* P = a.out + MAF_PR_HEADER;
    double* R = P + (size_t)nc * 1000;
    double* F1 = R + (size_t)nc * 1000;
    double* AP = F1 + (size_t)nc * 2000;
    double* NT = AP + (size_t)nc * niou;
    double* CM = NT + nc;
    int npres = 0;
    for (int c = 0; c < nc; ++c) npres += nt[c] > 0;
    for (int k = tid; k < 1000; k += CURVE_THREADS) {
        double acc = 0.0;
        bool first = true;
        for (int c = 0; c < nc; ++c)
            if (nt[c] > 0) { acc = first ? F1[(size_t)c * 1000 + k] : acc + F1[(size_t)c * 1000 + k]; first = false; }
        mean[k] = npres ? acc / (double)npres : 0.0;
    }
    for (int c = tid; c < nc; c += CURVE_THREADS) NT[c] = (double)nt[c];
    for (int q = tid; q < (nc + 1) * (nc + 1); q += CURVE_THREADS) CM[q] = (double)cm[q];
    __syncthreads();
    int idx = 0;
    {
        double best = mean[0];
        for (int k = 1; k < 1000; ++k)
            if (mean[k] >= best) { best = mean[k]; idx = k; }
    }
    // mp, mr, map50, map: numpy means over the present classes (col holds one column of them)
    double res[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < 4 && tid == 0; ++q) {
        int m = 0;
        for (int c = 0; c < nc; ++c) {
            if (nt[c] <= 0) continue;
            col[m++] = q == 0 ? P[(size_t)c * 1000 + idx] : q == 1 ? R[(size_t)c * 1000 + idx] : q == 2 ? AP[(size_t)c * niou]
                              : np_sum(AP + (size_t)c * niou, niou, 1) / (double)niou;
        }
        res[q] = npres ? np_sum(col, npres, 1) / (double)npres : 0.0;
    }
    if (tid == 0) {
        double* h = a.out;
        h[0] = (double)idx; h[1] = res[0]; h[2] = res[1]; h[3] = mean[idx]; h[4] = res[2]; h[5] = res[3];
        h[6] = (double)npres; h[7] = (double)a.state[1]; h[8] = (double)a.state[0];
    }
}

}  // namespace

extern "C" int64_t maf_pr_state_ints(int32_t nc) { return 2 + 2 * (int64_t)nc + (int64_t)(nc + 1) * (nc + 1); }

extern "C" int64_t maf_pr_out_doubles(int32_t nc, int32_t niou) {
    return MAF_PR_HEADER + 4 * 1000 * (int64_t)nc + (int64_t)nc * niou + nc + (int64_t)(nc + 1) * (nc + 1);
}

extern "C" int64_t maf_pr_workspace_bytes(int32_t nc, int32_t niou, int64_t capacity) {
    return 8 * (int64_t)(nc + 1) + (int64_t)niou * capacity * (4 + 8) + 256;
}

extern "C" int maf_pr_match(const float* rows, const int32_t* count, int32_t B, int32_t max_det, const float* targets, int32_t n_targets,
                            const float* img_params, int32_t H, int32_t W, const float* iouv, int32_t niou, int32_t nc, int32_t flags,
                            float cm_conf, float cm_iou, const int64_t* offs_in, int64_t* offs_out, int64_t* keys, uint16_t* masks,
                            int64_t capacity, int32_t* state, maf_stream_t stream) {
    MAF_REQUIRE(rows && count && iouv && offs_in && offs_out && keys && masks && state, "pr_match: null pointer");
    MAF_REQUIRE(n_targets == 0 || targets, "pr_match: null targets");
    MAF_REQUIRE((flags & MAF_PR_LABELS_XYXY) || img_params, "pr_match: null img_params");
    MAF_REQUIRE(B > 0 && max_det > 0 && max_det <= MAF_PR_MAX_DET, "pr_match: need 0 < max_det <= MAF_PR_MAX_DET and B > 0");
    MAF_REQUIRE(niou > 0 && niou <= 16 && nc > 0 && nc <= MAF_PR_MAX_CLASSES && n_targets >= 0 && H > 0 && W > 0, "pr_match: bad shape");
    MatchArgs a;
    a.rows = rows; a.count = count; a.targets = targets; a.img = img_params; a.iouv = iouv;
    a.offs_in = offs_in; a.offs_out = offs_out; a.keys = keys; a.masks = masks; a.state = state; a.capacity = capacity;
    a.B = B; a.max_det = max_det; a.n_targets = n_targets; a.H = H; a.W = W; a.niou = niou; a.nc = nc; a.flags = flags;
    a.cm_conf = cm_conf; a.cm_iou = cm_iou;
    hipLaunchKernelGGL(pr_match_kernel, dim3(B), dim3(MATCH_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return maf_check_hip(hipGetLastError(), "pr_match launch");
}

extern "C" int maf_pr_curves(const int64_t* sorted_keys, const int64_t* perm, const uint16_t* masks, int64_t capacity, const int32_t* state,
                             int32_t nc, int32_t niou, void* workspace, int64_t workspace_bytes, double* out, maf_stream_t stream) {
    MAF_REQUIRE(sorted_keys && perm && masks && state && workspace && out, "pr_curves: null pointer");
    MAF_REQUIRE(nc > 0 && nc <= MAF_PR_MAX_CLASSES && niou > 0 && niou <= 16 && capacity > 0, "pr_curves: bad shape");
    MAF_REQUIRE(workspace_bytes >= maf_pr_workspace_bytes(nc, niou, capacity), "pr_curves: workspace too small");
    MAF_REQUIRE(capacity < ((int64_t)1 << 31), "pr_curves: more than 2^31 - 1 records");
    CurveArgs a;
    char* ws = static_cast<char*>(workspace);
    a.skeys = sorted_keys; a.perm = perm; a.masks = masks; a.state = state; a.out = out; a.capacity = capacity; a.nc = nc; a.niou = niou;
    a.coff = reinterpret_cast<int64_t*>(ws);
    a.env = reinterpret_cast<double*>(ws + 8 * (int64_t)(nc + 1) + 64 - (8 * (int64_t)(nc + 1)) % 64);
    a.tpc = reinterpret_cast<int*>(a.env + (int64_t)niou * capacity);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pr_offsets_kernel, dim3(1), dim3(64), 0, st, a);
    hipLaunchKernelGGL(pr_curves_kernel, dim3(nc, niou), dim3(CURVE_THREADS), 0, st, a);
    hipLaunchKernelGGL(pr_summary_kernel, dim3(1), dim3(CURVE_THREADS), 0, st, a);
    return maf_check_hip(hipGetLastError(), "pr_curves launch");
}
