// COCO bbox mAP on the device — pycocotools' COCOeval (iouType 'bbox', useCats 1) as Evaler.eval_model (yolov6/core/evaler.py:276-364)
// runs it.  The rules are those of tests/cocoeval_ref.py: every IoU, precision, recall and score in fp64 without FMA contraction (this file
// is compiled with -ffp-contract=off), matches and envelopes bit for bit.
//
//   maf_coco_append      one launch per batch: maf_coco_rows' packed rows -> detection records (gt image index, category index, bbox and
//                        score rounded as post.convert_to_coco_format rounds them: rint(v * 1e3) / 1e3, rint(v * 1e5) / 1e5).
//   maf_coco_match       evaluateImg: one workgroup (one wave) per (image, category) cell, after a stable sort of the records by (cell,
//                        score descending).  The cell's first 100 detections, in that order, are matched greedily; lane a * 10 + t owns
//                        area range a and threshold t, so the 40 greedy scans of a cell run side by side over one fp64 IoU row in LDS.
//                        Per kept detection: its rank in the cell and the matched / ignored bits of the 40 (area, threshold) pairs; per
//                        cell: the non-ignored gt count of each area range.
//   maf_coco_accumulate  accumulate: after a stable sort of the kept detections by (category, score descending) (ties: image order, then
//                        rank in the cell — pycocotools' concatenate-then-mergesort order), one workgroup per (category, area, maxDet,
//                        threshold): a category's segment is split over 120 workgroups, and inside each over the threads in contiguous
//                        ranges.  Cumulative tp / fp, rc, pr, the right-to-left max envelope, searchsorted(rc, recThrs, 'left').
#include "maf_common.h"
#include "block_scan.h"

namespace {

constexpr int MATCH_THREADS = 64;            // one wave per cell
constexpr int ACC_THREADS = 512;
constexpr int T_ = MAF_COCO_T, A_ = MAF_COCO_A, M_ = MAF_COCO_M, R_ = MAF_COCO_R;
constexpr double EPS = 2.220446049250313e-16;   // np.spacing(1)

struct AppendArgs {
    const float* packed; const int32_t* total; const int32_t* img_index; const int32_t* cat_lut;
    int32_t* det_img; int32_t* det_cat; double* det_box; double* det_score;
    int64_t rows; int32_t B, n_lut;
};

__global__ __launch_bounds__(256) void coco_append_kernel(const AppendArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.rows) return;
    int img = -1, cat = -1;
    double box[4] = {0.0, 0.0, 0.0, 0.0}, score = 0.0;
    if (i < (int64_t)a.total[0]) {
        const float* p = a.packed + i * 7;
        const float fb = p[0], fc = p[1];
        if (fb >= 0.f && fb < (float)a.B) img = a.img_index[(int)fb];
        if (fc == fc && fc > -1.f && fc < (float)a.n_lut) cat = a.cat_lut[(int)fc];        // int(): truncation, as the host rows
        for (int k = 0; k < 4; ++k) box[k] = rint((double)p[2 + k] * 1000.0) / 1000.0;
        score = rint((double)p[6] * 100000.0) / 100000.0;
    }
    a.det_img[i] = img;
    a.det_cat[i] = cat;
    for (int k = 0; k < 4; ++k) a.det_box[i * 4 + k] = box[k];
    a.det_score[i] = score;
}

// first index in [0, n) with keys[index] >= v (keys ascending)
__device__ __forceinline__ int64_t lower_bound(const int64_t* keys, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct MatchArgs {
    const double* gt_box; const double* gt_area; const uint8_t* gt_flags; const int64_t* gt_off;
    const int64_t* cell_keys; const int64_t* order; const double* det_box;
    const uint8_t* img_sel; const int32_t* cat_map; const double* iou_thrs; const double* area_rng;
    int32_t* rank; uint64_t* mbits; uint64_t* ibits; int32_t* npig;
    int64_t n; int32_t I, K;
};

__global__ __launch_bounds__(MATCH_THREADS) void coco_match_kernel(const MatchArgs a) {
    __shared__ double gbox[MAF_COCO_MAX_GT][4];
    __shared__ double garea[MAF_COCO_MAX_GT];
    __shared__ double iou[MAF_COCO_MAX_GT];
    __shared__ uint8_t gflag[MAF_COCO_MAX_GT];
    __shared__ uint32_t gtm[T_ * A_][MAF_COCO_MAX_GT / 32];
    __shared__ int64_t s_d0, s_d1;
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x;
    const int img = (int)(c / a.K), cat = (int)(c % a.K);
    int32_t* np_out = a.npig + c * A_;
    if (!a.img_sel[img] || a.cat_map[cat] < 0) {
        if (lane < A_) np_out[lane] = 0;
        return;
    }
    const int64_t g0 = a.gt_off[c];
    const int ng = (int)min(a.gt_off[c + 1] - g0, (int64_t)MAF_COCO_MAX_GT);   // CocoGt refuses more on the host
    if (lane == 0) s_d0 = lower_bound(a.cell_keys, a.n, c);
    if (lane == 1) s_d1 = lower_bound(a.cell_keys, a.n, c + 1);
    for (int g = lane; g < ng; g += MATCH_THREADS) {
        for (int k = 0; k < 4; ++k) gbox[g][k] = a.gt_box[(g0 + g) * 4 + k];
        garea[g] = a.gt_area[g0 + g];
        gflag[g] = a.gt_flags[g0 + g];
    }
    for (int w = lane; w < T_ * A_ * (MAF_COCO_MAX_GT / 32); w += MATCH_THREADS) (&gtm[0][0])[w] = 0u;
    __syncthreads();
    const bool owner = lane < T_ * A_;                       // lane = area * 10 + threshold
    const int ar = owner ? lane / T_ : 0, th = owner ? lane % T_ : 0;
    const double lo = a.area_rng[2 * ar], hi = a.area_rng[2 * ar + 1];
    const double t = a.iou_thrs[th];
    const double start = fmin(t, 1.0 - 1e-10);
    if (lane < A_) {                                          // gts that are not ignored in area range `lane`
        const double l = a.area_rng[2 * lane], h = a.area_rng[2 * lane + 1];
        int cnt = 0;
        for (int g = 0; g < ng; ++g) cnt += !((gflag[g] & MAF_COCO_GT_CROWD) || garea[g] < l || garea[g] > h);
        np_out[lane] = cnt;
    }
    const int64_t d0 = s_d0;
    const int nd = (int)min(s_d1 - d0, (int64_t)MAF_COCO_MAX_DETS);
    for (int d = 0; d < nd; ++d) {
        const double* db = a.det_box + a.order[d0 + d] * 4;
        const double dx = db[0], dy = db[1], dw = db[2], dh = db[3];
        const double da = dw * dh;
        for (int g = lane; g < ng; g += MATCH_THREADS) {      // bbIou of pycocotools' maskApi.c
            const double gx = gbox[g][0], gy = gbox[g][1], gw = gbox[g][2], gh = gbox[g][3];
            double v = 0.0;
            const double w = fmin(dw + dx, gw + gx) - fmax(dx, gx);
            if (w > 0.0) {
                const double h = fmin(dh + dy, gh + gy) - fmax(dy, gy);
                if (h > 0.0) {
                    const double i = w * h;
                    const double u = (gflag[g] & MAF_COCO_GT_CROWD) ? da : da + gw * gh - i;
                    v = i / u;
                }
            }
            iou[g] = v;
        }
        __syncthreads();
        bool matched = false, ignored = false;
        if (owner) {
            double best = start;
            int m = -1, mig = 0;
            // the gts in _ignore-sorted order: the non-ignored ones in JSON order, then the ignored ones; a match among the first stops the
            // scan at the first ignored gt
            for (int pass = 0; pass < 2 && !(pass == 1 && m >= 0); ++pass)
                for (int g = 0; g < ng; ++g) {
                    const int crowd = gflag[g] & MAF_COCO_GT_CROWD;
                    const int ig = crowd || garea[g] < lo || garea[g] > hi;
                    if (ig != pass) continue;
                    if (((gtm[lane][g >> 5] >> (g & 31)) & 1u) && !crowd) continue;
                    if (iou[g] < best) continue;
                    best = iou[g];
                    m = g;
                    mig = ig;
                }
            if (m >= 0) {
                gtm[lane][m >> 5] |= 1u << (m & 31);
                matched = gflag[m] & MAF_COCO_GT_IDNZ;       // dtMatches holds the gt's id: id 0 reads as unmatched
                ignored = mig;
            }
            if (!matched && (da < lo || da > hi)) ignored = true;
        }
        const uint64_t mb = __ballot(matched), ib = __ballot(ignored);
        if (lane == 0) {
            a.rank[d0 + d] = d;
            a.mbits[d0 + d] = mb;
            a.ibits[d0 + d] = ib;
        }
        __syncthreads();
    }
}

struct AccArgs {
    const int64_t* keys; const int32_t* rank; const uint64_t* mbits; const uint64_t* ibits; const double* score;
    const int32_t* npig; const uint8_t* img_sel; const int32_t* cat_of; const double* rec_thrs; const int32_t* max_dets;
    double* precision; double* recall; double* scores;
    int64_t n; int32_t I, K, Kp;
};

struct Cnt3 {
    int nd, tp, fp;
    __device__ Cnt3& operator+=(const Cnt3& o) { nd += o.nd; tp += o.tp; fp += o.fp; return *this; }
    __device__ Cnt3 operator-(const Cnt3& o) const { return Cnt3{nd - o.nd, tp - o.tp, fp - o.fp}; }
};

__device__ __forceinline__ double pr_of(int tp, int fp) { return (double)tp / ((double)fp + (double)tp + EPS); }

__global__ __launch_bounds__(ACC_THREADS) void coco_accumulate_kernel(const AccArgs a) {
    __shared__ Cnt3 sh3[ACC_THREADS];
    __shared__ double shd[ACC_THREADS];
    __shared__ int cr[R_];
    __shared__ double q[R_], ss[R_];
    __shared__ int s_npig;
    __shared__ int64_t s_s0, s_s1;
    const int tid = threadIdx.x;
    const int id = blockIdx.x;                               // ((k * A + a) * M + m) * T + t
    const int t = id % T_, m = (id / T_) % M_, ar = (id / (T_ * M_)) % A_, kp = id / (T_ * M_ * A_);
    const int k = a.cat_of[kp];
    const int bit = ar * T_ + t;
    const int maxdet = a.max_dets[m];
    // npig: the category's non-ignored gts of area range ar over the selected images
    int cnt = 0;
    if (k >= 0)
        for (int i = tid; i < a.I; i += ACC_THREADS) cnt += a.img_sel[i] ? a.npig[((int64_t)i * a.K + k) * A_ + ar] : 0;
    const Cnt3 tot0 = block_excl_sum<ACC_THREADS>(Cnt3{cnt, 0, 0}, sh3);
    if (tid == ACC_THREADS - 1) {
        s_npig = tot0.nd + cnt;
        s_s0 = lower_bound(a.keys, a.n, kp);
        s_s1 = lower_bound(a.keys, a.n, (int64_t)kp + 1);
    }
    if (tid < R_) { q[tid] = 0.0; ss[tid] = 0.0; }
    __syncthreads();
    const int npig = s_npig;
    const size_t KAM = (size_t)a.Kp * A_ * M_;
    const size_t oqk = (size_t)kp * A_ * M_ + (size_t)ar * M_ + m;                // [t][r][k][a][m] without the t / r terms
    if (npig == 0) {                                          // pycocotools `continue`s: -1 stays
        for (int r = tid; r < R_; r += ACC_THREADS) {
            a.precision[((size_t)t * R_ + r) * KAM + oqk] = -1.0;
            a.scores[((size_t)t * R_ + r) * KAM + oqk] = -1.0;
        }
        if (tid == 0) a.recall[(size_t)t * KAM + oqk] = -1.0;
        return;
    }
    if (tid < R_) {                                           // smallest tp count c with c / npig >= recThrs[r] (rc is tp / npig)
        const double thr = a.rec_thrs[tid];
        int l = 0, h = npig;
        while (l < h) {
            const int mid = (l + h) >> 1;
            if ((double)mid / (double)npig >= thr) h = mid; else l = mid + 1;
        }
        cr[tid] = l;
    }
    const int64_t s0 = s_s0, L = s_s1 - s_s0;
    const int64_t chunk = (L + ACC_THREADS - 1) / ACC_THREADS;
    const int64_t i0 = min(L, chunk * tid), i1 = min(L, i0 + chunk);
    // 1. this thread's counts -> its starting cumulative sums
    Cnt3 own{0, 0, 0};
    for (int64_t i = i0; i < i1; ++i) {
        if (a.rank[s0 + i] >= maxdet) continue;
        const int mb = (a.mbits[s0 + i] >> bit) & 1, ib = (a.ibits[s0 + i] >> bit) & 1;
        own.nd += 1;
        own.tp += mb & !ib;
        own.fp += !mb & !ib;
    }
    const Cnt3 pre = block_excl_sum<ACC_THREADS>(own, sh3);
    if (tid == ACC_THREADS - 1) {
        const int nd = pre.nd + own.nd, tp = pre.tp + own.tp;
        a.recall[(size_t)t * KAM + oqk] = nd ? (double)tp / (double)npig : 0.0;
    }
    // 2. the max of pr over this thread's range, then over the ranges after it
    double mx = 0.0;
    {
        int tp = pre.tp, fp = pre.fp;
        for (int64_t i = i0; i < i1; ++i) {
            if (a.rank[s0 + i] >= maxdet) continue;
            const int mb = (a.mbits[s0 + i] >> bit) & 1, ib = (a.ibits[s0 + i] >> bit) & 1;
            tp += mb & !ib;
            fp += !mb & !ib;
            mx = fmax(mx, pr_of(tp, fp));
        }
    }
    double env = block_suffix_max_after<ACC_THREADS>(mx, shd);
    // 3. right to left over the range: the envelope at each position; the positions searchsorted lands on write q / ss
    {
        int nd = pre.nd + own.nd, tp = pre.tp + own.tp, fp = pre.fp + own.fp;
        for (int64_t i = i1 - 1; i >= i0; --i) {
            if (a.rank[s0 + i] >= maxdet) continue;
            env = fmax(env, pr_of(tp, fp));
            const int mb = (a.mbits[s0 + i] >> bit) & 1, ib = (a.ibits[s0 + i] >> bit) & 1;
            const int is_tp = mb & !ib;
            // first index with rc >= recThrs[r]: index 0 for cr == 0, else the position of the cr-th true positive
            if (nd == 1)
                for (int r = 0; r < R_ && cr[r] == 0; ++r) { q[r] = env; ss[r] = a.score[s0 + i]; }
            if (is_tp) {
                int r = 0;
                while (r < R_ && cr[r] < tp) ++r;
                for (; r < R_ && cr[r] == tp; ++r) { q[r] = env; ss[r] = a.score[s0 + i]; }
            }
            nd -= 1;
            tp -= is_tp;
            fp -= !mb & !ib;
        }
    }
    __syncthreads();
    for (int r = tid; r < R_; r += ACC_THREADS) {
        a.precision[((size_t)t * R_ + r) * KAM + oqk] = q[r];
        a.scores[((size_t)t * R_ + r) * KAM + oqk] = ss[r];
    }
}

}  // namespace

extern "C" int maf_coco_append(const float* packed, const int32_t* total, int64_t rows, const int32_t* img_index, int32_t B,
                               const int32_t* cat_lut, int32_t n_lut, int32_t* det_img, int32_t* det_cat, double* det_box, double* det_score,
                               maf_stream_t stream) {
    MAF_REQUIRE(packed && total && img_index && det_img && det_cat && det_box && det_score, "coco_append: null pointer");
    MAF_REQUIRE(rows > 0 && B > 0 && n_lut >= 0 && (n_lut == 0 || cat_lut), "coco_append: bad shape");
    AppendArgs a;
    a.packed = packed; a.total = total; a.img_index = img_index; a.cat_lut = cat_lut;
    a.det_img = det_img; a.det_cat = det_cat; a.det_box = det_box; a.det_score = det_score;
    a.rows = rows; a.B = B; a.n_lut = n_lut;
    hipLaunchKernelGGL(coco_append_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return maf_check_hip(hipGetLastError(), "coco_append launch");
}

extern "C" int maf_coco_match(const double* gt_box, const double* gt_area, const uint8_t* gt_flags, const int64_t* gt_off,
                              const int64_t* cell_keys, const int64_t* order, const double* det_box, int64_t n, const uint8_t* img_sel,
                              const int32_t* cat_map, int32_t I, int32_t K, const double* iou_thrs, const double* area_rng, int32_t* rank,
                              uint64_t* mbits, uint64_t* ibits, int32_t* npig, maf_stream_t stream) {
    MAF_REQUIRE(gt_off && cell_keys && order && det_box && img_sel && cat_map && iou_thrs && area_rng && rank && mbits && ibits && npig,
                "coco_match: null pointer");
    MAF_REQUIRE(I > 0 && K > 0 && n > 0 && (int64_t)I * K < ((int64_t)1 << 31), "coco_match: bad shape");
    MatchArgs a;
    a.gt_box = gt_box; a.gt_area = gt_area; a.gt_flags = gt_flags; a.gt_off = gt_off; a.cell_keys = cell_keys; a.order = order;
    a.det_box = det_box; a.img_sel = img_sel; a.cat_map = cat_map; a.iou_thrs = iou_thrs; a.area_rng = area_rng;
    a.rank = rank; a.mbits = mbits; a.ibits = ibits; a.npig = npig; a.n = n; a.I = I; a.K = K;
    hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)((int64_t)I * K)), dim3(MATCH_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return maf_check_hip(hipGetLastError(), "coco_match launch");
}

extern "C" int maf_coco_accumulate(const int64_t* cat_keys, const int32_t* rank, const uint64_t* mbits, const uint64_t* ibits, const double* score,
                                   int64_t n, const int32_t* npig, const uint8_t* img_sel, const int32_t* cat_of, int32_t I, int32_t K, int32_t Kp,
                                   const double* rec_thrs, const int32_t* max_dets, double* precision, double* recall, double* scores,
                                   maf_stream_t stream) {
    MAF_REQUIRE(cat_keys && rank && mbits && ibits && score && npig && img_sel && cat_of && rec_thrs && max_dets && precision && recall && scores,
                "coco_accumulate: null pointer");
    MAF_REQUIRE(I > 0 && K > 0 && Kp > 0 && n > 0 && n < ((int64_t)1 << 31), "coco_accumulate: bad shape");
    AccArgs a;
    a.keys = cat_keys; a.rank = rank; a.mbits = mbits; a.ibits = ibits; a.score = score; a.npig = npig; a.img_sel = img_sel; a.cat_of = cat_of;
    a.rec_thrs = rec_thrs; a.max_dets = max_dets; a.precision = precision; a.recall = recall; a.scores = scores;
    a.n = n; a.I = I; a.K = K; a.Kp = Kp;
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)Kp * A_ * M_ * T_), dim3(ACC_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return maf_check_hip(hipGetLastError(), "coco_accumulate launch");
}
