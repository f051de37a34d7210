// Loss of the validation epoch on gfx950: OrienMaskYOLOMultiScaleLoss's values (eval/orienmask_yolo_loss.py:62-264,
// eval/base.py:27-40) for up to three scales in four launches, with no host synchronisation and fixed-order sums.
//
//   loss_match_kernel   one lane per (GT, scale): anchor_ious against the scale's grid_all_anchors, argmax (first maximum),
//                       the positive cell (a, gy, gx) with clamped floor, txy / twh / bbox_pos_scale, and the orientation ROI
//                       (valid_region / center_region, round half to even).  Written to the workspace (LossGt); no atomics.
//   loss_box_kernel     one lane per prediction cell (b, a, gy, gx) of a scale, the image's GTs in LDS: decode, bbox_ious
//                       against ALL the image's GTs (the ignore mask), the cell's winner among the GTs matched to it, the BCE /
//                       MSE terms and the box metrics.
//   loss_orien_kernel   one workgroup per (scale, image, anchor, 16 x 64 pixel tile): the image's instances matched to that
//                       anchor whose ROI meets the tile are culled into LDS in collate order (ballot / prefix); each pixel then
//                       walks them in order -- the reference's per-instance update is pixel-local, so this is an exact
//                       restatement -- divides by anchor / 2 and by the count, and adds the x4 bilinear up-sampled SmoothL1 and
//                       accuracy terms.  A tile no ROI meets exits at once.
//   loss_reduce_kernel  one workgroup per scale: the workgroup partials (doubles) summed in a fixed order, the reference's
//                       normalisations in float32, the per-item weights.
//
// The backward (om_loss_backward, two launches after om_loss on the same inputs):
//   loss_box_grad_kernel    one lane per prediction cell: the forward's decode / ignore / winner again, then the gradient of
//                           all 5 + C channels of the cell (zeros included) along the BCE / sigmoid / MSE chain.
//   loss_orien_grad_kernel  one workgroup per (scale, image, anchor, 16 x 16 quarter-resolution tile): targets and
//                           d loss / d(up-sampled head) of the tile plus a 2-pixel halo into LDS, then each quarter pixel gathers
//                           the up-sample's adjoint in a fixed order.  No atomics, no full-resolution scratch in memory.
//
// Duplicate positives (two GTs of one image on the same (a, gy, gx)): the reference's index_put_ writes are last-writer-wins
// on torch-CPU and unspecified on CUDA.  Here: txy, twh, bbox_pos_scale and tiou come from the HIGHEST GT index on the cell, tcls is
// the UNION of their classes (different class indices are different elements, so every write survives) -- the CPU answer.
//
// Elementary functions (probed on torch-CPU 2.10, x86-64 AVX-512, one thread, against the loss's own views):
//   * pred_bbox[..., 0:2].sigmoid() and [..., 4].sigmoid(): bit-identical to the scalar-view sigmoid ref_math.h restates
//     (glibc expf); pred_bbox[..., 5:].sigmoid() has the postprocess's row layout (rows of C at stride 5 + C): Sleef for
//     the first (C / 32) * 32 classes, glibc for the tail -- restated bit-exactly (ref_math.h).
//   * pred_wh.exp(): MKL's vsExp, as in the postprocess (1.1 % of inputs differ from the correctly rounded value by one ulp):
//     NOT restated; the correctly rounded value is used.  torch.log(gt_wh / anchor) (twh): vsLn, likewise correctly rounded
//     here (within one ulp).
//   * BCELoss: (t - 1) * max(log1p(-p), -100) - t * max(log(p), -100) with glibc's log1pf / logf (0 mismatches on 2e4
//     probes): evaluated here in double and rounded once (the correctly rounded value; glibc differs by one ulp on ~1 %).
// Loss terms therefore agree with the reference to ~1e-7 relative, the targets that use only + - * / and round bit for bit.
//
// This file is compiled with -ffp-contract=off: every float32 operation rounds as the reference's tensor op does.
#include "om_common.h"
#include "ref_math.h"
#include "bilinear.h"

#include <algorithm>

namespace om {

constexpr int LOSS_BOX_THREADS = 256;
constexpr int LOSS_OR_THREADS = 256;
constexpr int LOSS_TILE_H = 16, LOSS_TILE_W = 64;
constexpr int LOSS_BOX_VALS = 16;       // doubles per box partial
constexpr int LOSS_OR_VALS = 8;         // doubles per orientation partial

struct LossGt {                 // one GT at one scale (grid units unless stated)
    int key;                    // a * nH * nW + gy * nW + gx of its positive cell, -1: matched at another scale
    int a;                      // anchor within the scale
    int x1, x2, y1, y2;         // ROI [x1, x2) x [y1, y2), pixels
    float px, py, cw, ch;       // centre (pixels), center_wh
    float gx, gy, gw, gh;       // box
    float tx, ty, tw, th, pscale;
    int cls;
};

struct LossParams {
    om_loss_cfg cfg;
    const float* bbox[OM_MAX_SCALES];
    const float* orien[OM_MAX_SCALES];
    int B, N;
    const float* gt_bbox;
    const int64_t* gt_cls;
    const int64_t* gt_index;
    const uint8_t* gt_mask;
    LossGt* gts;                // [scale][N]
    double* box_part;           // [scale][B][box_blocks][LOSS_BOX_VALS]
    double* or_part;            // [scale][B * 3][tiles][LOSS_OR_VALS]
    int box_blocks, tiles, tiles_x;
    float* result;
    // om_loss_targets: one scale's targets (any may be null)
    int tgt_scale;
    float *t_pos, *t_neg, *t_pscale, *t_txy, *t_twh, *t_tiou, *t_tcls, *t_torien;
    int* t_omask;
};

__device__ __forceinline__ void set_flag(const LossParams& p, int bit) {
    atomicOr(reinterpret_cast<int*>(p.result + OM_LOSS_FLAG_OFF), bit);
}

// the image's GT range [g0, g0 + n), clamped so that no read leaves the arrays; a bad prefix was flagged by the match kernel
__device__ __forceinline__ void image_range(const LossParams& p, int b, int& g0, int& n) {
    long long lo = p.gt_index[b], hi = p.gt_index[b + 1];
    lo = lo < 0 ? 0 : lo > p.N ? p.N : lo;
    hi = hi < lo ? lo : hi > p.N ? p.N : hi;
    g0 = (int)lo;
    n = (int)(hi - lo);
    if (n > OM_LOSS_MAX_GT) n = OM_LOSS_MAX_GT;
}

__device__ __forceinline__ float minf_(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float maxf_(float a, float b) { return b > a ? b : a; }

// BCELoss element: (t - 1) * max(log1p(-p), -100) - t * max(log(p), -100)
__device__ __forceinline__ float bce(float pr, float t) {
    const float l1 = maxf_((float)log1p(-(double)pr), -100.0f);
    const float l0 = maxf_((float)log((double)pr), -100.0f);
    return (t - 1.0f) * l1 - t * l0;
}

// ------------------------------------------------------------------------------------------------
// match: orienmask_yolo_loss.py:175 (gt_bbox * [nW, nH, nW, nH]), :190-230 (matching, box targets, ROI)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void loss_match_kernel(const LossParams p) {
    const int s = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (s == 0 && n <= p.B) {           // gt_index must be a prefix of [0, N] with at most OM_LOSS_MAX_GT per image
        const long long v = p.gt_index[n];
        bool bad = v < 0 || v > p.N || (n == 0 && v != 0) || (n == p.B && v != p.N);
        if (n > 0) {
            const long long d = v - p.gt_index[n - 1];
            bad = bad || d < 0 || d > OM_LOSS_MAX_GT;
        }
        if (bad) set_flag(p, OM_LOSS_FLAG_TOO_MANY_GT);
    }
    if (n >= p.N) return;
    const om_loss_cfg& c = p.cfg;
    const int nH = c.grid_h[s], nW = c.grid_w[s];
    const float fW = (float)nW, fH = (float)nH;
    const float bx = p.gt_bbox[4 * n] * fW, by = p.gt_bbox[4 * n + 1] * fH;
    const float bw = p.gt_bbox[4 * n + 2] * fW, bh = p.gt_bbox[4 * n + 3] * fH;
    const float sw = (float)c.image_w / fW, sh = (float)c.image_h / fH;       // scale_wh
    const long long cl = p.gt_cls[n];
    if (s == 0 && (cl < 0 || cl >= c.num_classes)) set_flag(p, OM_LOSS_FLAG_BAD_CLASS);
    // anchor_ious(gt_wh, grid_all_anchors).argmax(dim=1): the first maximum
    int best = 0;
    float best_iou = 0.0f;
    for (int k = 0; k < c.num_anchors_total; ++k) {
        const float aw = c.anchor_w[k] / sw, ah = c.anchor_h[k] / sh;
        const float inter = minf_(bw, aw) * minf_(bh, ah);
        const float uni = (bw * bh + aw * ah) - inter;
        const float iou = inter / uni;
        if (k == 0 || iou > best_iou) {
            best = k;
            best_iou = iou;
        }
    }
    LossGt g;
    g.a = -1;
    for (int a = 0; a < c.anchors_of_scale[s]; ++a)
        if (c.anchor_mask[s][a] == best && g.a < 0) g.a = a;
    g.cls = (cl < 0 || cl >= c.num_classes) ? -1 : (int)cl;
    g.gx = bx; g.gy = by; g.gw = bw; g.gh = bh;
    const int gxi = (int)minf_(maxf_(floorf(bx), 0.0f), (float)(nW - 1));
    const int gyi = (int)minf_(maxf_(floorf(by), 0.0f), (float)(nH - 1));
    g.key = g.a < 0 ? -1 : (g.a * nH + gyi) * nW + gxi;
    g.pscale = 2.0f - (bw * bh) / (float)(nW * nH);
    g.tx = bx - (float)gxi;
    g.ty = by - (float)gyi;
    const int ag = g.a < 0 ? 0 : c.anchor_mask[s][g.a];
    g.tw = (float)log((double)(bw / (c.anchor_w[ag] / sw)));
    g.th = (float)log((double)(bh / (c.anchor_h[ag] / sh)));
    // orientation ROI (pixels)
    const float vr = c.valid_region, cr = c.center_region;
    g.px = bx * sw;
    g.py = by * sh;
    const float vw = (bw * vr + 0.5f) * sw, vh = (bh * vr + 0.5f) * sh;
    g.cw = vw / vr * cr;
    g.ch = vh / vr * cr;
    const float xm = (float)(c.image_w - 1), ym = (float)(c.image_h - 1);
    g.x1 = (int)rintf(minf_(maxf_(g.px - vw, 0.0f), xm));
    g.x2 = (int)rintf(minf_(maxf_(g.px + vw, 0.0f), xm)) + 1;
    g.y1 = (int)rintf(minf_(maxf_(g.py - vh, 0.0f), ym));
    g.y2 = (int)rintf(minf_(maxf_(g.py + vh, 0.0f), ym)) + 1;
    p.gts[(size_t)s * p.N + n] = g;
}

// deterministic workgroup sum of V doubles per lane (shuffle tree, then the waves in order); valid in thread 0
template <int V, int THREADS>
__device__ __forceinline__ void block_sum(double (&v)[V], double (*s_red)[V]) {
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] += __shfl_xor(v[i], off);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int i = 0; i < V; ++i) s_red[w][i] = v[i];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int ww = 1; ww < THREADS / 64; ++ww)
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] += s_red[ww][i];
}

// ------------------------------------------------------------------------------------------------
// box: orienmask_yolo_loss.py:88-124 (decode), :183-209 (ignore, positives), :122-135 (terms), :148-164 (metrics)
// grid (box_blocks, B, scales)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LOSS_BOX_THREADS) void loss_box_kernel(const LossParams p) {
    __shared__ float4 s_box[OM_LOSS_MAX_GT];
    __shared__ int s_key[OM_LOSS_MAX_GT];
    __shared__ int s_cls[OM_LOSS_MAX_GT];
    __shared__ double s_red[LOSS_BOX_THREADS / 64][LOSS_BOX_VALS];
    const int s = blockIdx.z, b = blockIdx.y;
    const om_loss_cfg& c = p.cfg;
    double* part = p.box_part + (((size_t)s * p.B + b) * p.box_blocks + blockIdx.x) * LOSS_BOX_VALS;
    const int nH = c.grid_h[s], nW = c.grid_w[s], A = c.anchors_of_scale[s], C = c.num_classes;
    const int ncell = A * nH * nW;
    const bool debug = p.tgt_scale >= 0;
    if (s >= c.num_scales || (debug && s != p.tgt_scale) || (int)blockIdx.x * LOSS_BOX_THREADS >= ncell) {
        if (threadIdx.x < LOSS_BOX_VALS) part[threadIdx.x] = 0.0;
        return;
    }
    int g0, ng;
    image_range(p, b, g0, ng);
    const LossGt* gts = p.gts + (size_t)s * p.N + g0;
    for (int j = threadIdx.x; j < ng; j += LOSS_BOX_THREADS) {
        const LossGt& g = gts[j];
        s_box[j] = make_float4(g.gx, g.gy, g.gw, g.gh);
        s_key[j] = g.key;
        s_cls[j] = g.cls;
    }
    __syncthreads();
    double v[LOSS_BOX_VALS];
#pragma unroll
    for (int i = 0; i < LOSS_BOX_VALS; ++i) v[i] = 0.0;
    const int cell = blockIdx.x * LOSS_BOX_THREADS + threadIdx.x;
    if (cell < ncell) {
        const int a = cell / (nH * nW), rem = cell - a * (nH * nW);
        const int gy = rem / nW, gx = rem - gy * nW;
        const int64_t* st = c.bbox_stride[s];
        const float* hp = p.bbox[s] + b * st[0] + (int64_t)a * (5 + C) * st[1] + gy * st[2] + gx * st[3];
        const float vx = hp[0], vy = hp[st[1]], vw = hp[2 * st[1]], vh = hp[3 * st[1]], vo = hp[4 * st[1]];
        if (!isfinite(vw) || !isfinite(vh)) set_flag(p, OM_LOSS_FLAG_NONFINITE_WH);
        const int ag = c.anchor_mask[s][a];
        const float sw = (float)c.image_w / (float)nW, sh = (float)c.image_h / (float)nH;
        const float sx = sigmoid_scalar_ref(vx), sy = sigmoid_scalar_ref(vy), so = sigmoid_scalar_ref(vo);
        const float x = sx + (float)gx, y = sy + (float)gy;
        const float w = expf_cr(vw) * (c.anchor_w[ag] / sw), h = expf_cr(vh) * (c.anchor_h[ag] / sh);
        const float b1x1 = x - w / 2.0f, b1y1 = y - h / 2.0f, b1x2 = x + w / 2.0f, b1y2 = y + h / 2.0f;
        const float area1 = (b1x2 - b1x1) * (b1y2 - b1y1);
        bool ignore = false;
        int win = -1, nmatch = 0;
        float tiou = 0.0f;
        int cls4[4];
        for (int j = 0; j < ng; ++j) {
            const float4 g = s_box[j];
            const float b2x1 = g.x - g.z / 2.0f, b2y1 = g.y - g.w / 2.0f, b2x2 = g.x + g.z / 2.0f, b2y2 = g.y + g.w / 2.0f;
            float dx = minf_(b1x2, b2x2) - maxf_(b1x1, b2x1);
            float dy = minf_(b1y2, b2y2) - maxf_(b1y1, b2y1);
            dx = dx < 0.0f ? 0.0f : dx;
            dy = dy < 0.0f ? 0.0f : dy;
            const float inter = dx * dy;
            const float area2 = (b2x2 - b2x1) * (b2y2 - b2y1);
            const float iou = inter / ((area1 + area2) - inter);
            ignore = ignore || iou > c.obj_ignore_threshold;
            if (s_key[j] == cell) {
                win = j;
                tiou = iou;
                if (nmatch < 4) cls4[nmatch] = s_cls[j];
                ++nmatch;
            }
        }
        const bool pos = win >= 0, neg = !pos && !ignore;
        float tx = 0.f, ty = 0.f, tw = 0.f, th = 0.f, ps = 0.f;
        if (pos) {
            const LossGt& g = gts[win];
            tx = g.tx; ty = g.ty; tw = g.tw; th = g.th; ps = g.pscale;
        }
        if (pos) {
            v[0] = (double)(bce(sx, tx) * ps) + (double)(bce(sy, ty) * ps);
            const float dw = vw - tw, dh = vh - th;
            v[1] = (double)((dw * dw) * ps) + (double)((dh * dh) * ps);
            v[2] = (double)bce(so, 1.0f);
            v[6] = (double)so;
            v[8] = (double)tiou;
            v[9] = 1.0;
            v[11] = tiou > 0.5f ? 1.0 : 0.0;
            v[12] = tiou > 0.75f ? 1.0 : 0.0;
        }
        if (neg) {
            v[3] = (double)bce(so, 0.0f);
            v[7] = (double)so;
            v[10] = 1.0;
        }
        const bool want_cls = debug && p.t_tcls;
        if (pos || want_cls) {
            const float* cp = hp + 5 * st[1];
            double lc = 0.0, conf = 0.0;
            for (int k = 0; k < C; ++k) {
                bool on = false;
                if (pos) {
                    if (nmatch <= 4) {
                        for (int m = 0; m < nmatch && m < 4; ++m) on = on || cls4[m] == k;
                    } else {
                        for (int j = 0; j < ng; ++j) on = on || (s_key[j] == cell && s_cls[j] == k);
                    }
                }
                const float t = on ? c.label_on : c.label_smooth;
                if (want_cls) p.t_tcls[((size_t)b * A * nH * nW + cell) * C + k] = t;
                if (pos) {
                    const float sc = sigmoid_class_ref(cp[k * st[1]], k, C);
                    lc += (double)bce(sc, t);
                    if (t > 0.5f) conf += (double)sc;
                }
            }
            v[4] = lc;
            v[5] = conf;
        }
        if (debug) {
            const size_t o = (size_t)b * A * nH * nW + cell;
            if (p.t_pos) p.t_pos[o] = pos ? 1.0f : 0.0f;
            if (p.t_neg) p.t_neg[o] = neg ? 1.0f : 0.0f;
            if (p.t_pscale) p.t_pscale[o] = ps;
            if (p.t_txy) { p.t_txy[2 * o] = tx; p.t_txy[2 * o + 1] = ty; }
            if (p.t_twh) { p.t_twh[2 * o] = tw; p.t_twh[2 * o + 1] = th; }
            if (p.t_tiou) p.t_tiou[o] = pos ? tiou : 0.0f;
        }
    }
    block_sum<LOSS_BOX_VALS, LOSS_BOX_THREADS>(v, s_red);
    if (threadIdx.x == 0)
        for (int i = 0; i < LOSS_BOX_VALS; ++i) part[i] = v[i];
}

// ------------------------------------------------------------------------------------------------
// orientation: orienmask_yolo_loss.py:212-255 (targets), :86 + :137-145 (up-sampled SmoothL1), :158-162 (accuracy)
// grid (tiles, B * 3, scales)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LOSS_OR_THREADS) void loss_orien_kernel(const LossParams p) {
    __shared__ int4 s_roi[OM_LOSS_MAX_GT];
    __shared__ float4 s_geo[OM_LOSS_MAX_GT];
    __shared__ int s_idx[OM_LOSS_MAX_GT];
    __shared__ int s_n;
    __shared__ double s_red[LOSS_OR_THREADS / 64][LOSS_OR_VALS];
    const int s = blockIdx.z, b = blockIdx.y / 3, a = blockIdx.y - 3 * (blockIdx.y / 3);
    const om_loss_cfg& c = p.cfg;
    double* part = p.or_part + (((size_t)s * p.B * 3 + blockIdx.y) * p.tiles + blockIdx.x) * LOSS_OR_VALS;
    const bool debug = p.tgt_scale >= 0;
    if (s >= c.num_scales || a >= c.anchors_of_scale[s] || (debug && s != p.tgt_scale)) {
        if (threadIdx.x < LOSS_OR_VALS) part[threadIdx.x] = 0.0;
        return;
    }
    const int H = c.image_h, W = c.image_w;
    const int ty0 = (blockIdx.x / p.tiles_x) * LOSS_TILE_H, tx0 = (blockIdx.x % p.tiles_x) * LOSS_TILE_W;
    int g0, ng;
    image_range(p, b, g0, ng);
    const LossGt* gts = p.gts + (size_t)s * p.N + g0;
    if (threadIdx.x < 64) {         // cull in collate order: one wave, ballot + prefix
        const int lane = threadIdx.x;
        int base = 0;
        for (int j0 = 0; j0 < ng; j0 += 64) {
            const int j = j0 + lane;
            bool mine = false;
            LossGt g;
            if (j < ng) {
                g = gts[j];
                mine = g.key >= 0 && g.a == a && g.x1 < tx0 + LOSS_TILE_W && g.x2 > tx0 && g.y1 < ty0 + LOSS_TILE_H && g.y2 > ty0;
            }
            const unsigned long long votes = __ballot(mine);
            if (mine) {
                const int slot = base + __popcll(votes & ((1ull << lane) - 1ull));
                s_roi[slot] = make_int4(g.x1, g.x2, g.y1, g.y2);
                s_geo[slot] = make_float4(g.px, g.py, g.cw, g.ch);
                s_idx[slot] = g0 + j;
            }
            base += __popcll(votes);
        }
        if (lane == 0) s_n = base;
    }
    __syncthreads();
    const int n_inst = s_n;
    const bool want_t = debug && (p.t_omask || p.t_torien);
    if (n_inst == 0 && !want_t) {
        if (threadIdx.x < LOSS_OR_VALS) part[threadIdx.x] = 0.0;
        return;
    }
    const int ag = c.anchor_mask[s][a];
    const float haw = c.anchor_w[ag] / 2.0f, hah = c.anchor_h[ag] / 2.0f;      // pixel_anchors / 2
    const int oh = H / 4, ow = W / 4;
    const int64_t* ost = c.orien_stride[s];
    const float* pxp = p.orien[s] + b * ost[0] + (int64_t)(2 * a) * ost[1];
    const float* pyp = pxp + ost[1];
    double v[LOSS_OR_VALS];
#pragma unroll
    for (int i = 0; i < LOSS_OR_VALS; ++i) v[i] = 0.0;
    const int px = tx0 + (threadIdx.x & 63);
    for (int r = threadIdx.x >> 6; r < LOSS_TILE_H; r += LOSS_OR_THREADS / 64) {
        const int py = ty0 + r;
        if (px >= W || py >= H) continue;
        int state = 0;
        float t0 = 0.0f, t1 = 0.0f;
        const float fx = (float)px, fy = (float)py;
        for (int i = 0; i < n_inst; ++i) {
            const int4 roi = s_roi[i];
            if (px < roi.x || px >= roi.y || py < roi.z || py >= roi.w) continue;
            const float4 g = s_geo[i];
            const float ox = fx - g.x, oy = fy - g.y;
            if (p.gt_mask[((size_t)s_idx[i] * H + py) * W + px]) {
                state = -1;
                t0 = ox;
                t1 = oy;
            } else if (state >= 0) {
                state += 1;
                const float lx = maxf_(fabsf(ox), 1e-8f), ly = maxf_(fabsf(oy), 1e-8f);
                const float qx = maxf_(g.z / lx, 1.0f), qy = maxf_(g.w / ly, 1.0f);
                const float q = minf_(qx, qy) - 1.0f;
                const float sgx = ox > 0.0f ? 1.0f : ox < 0.0f ? -1.0f : 0.0f;
                const float sgy = oy > 0.0f ? 1.0f : oy < 0.0f ? -1.0f : 0.0f;
                t0 = t0 + (q * sgx) * lx;
                t1 = t1 + (q * sgy) * ly;
            }
        }
        t0 = t0 / haw;
        t1 = t1 / hah;
        const float den = state < 0 ? -1.0f : state == 0 ? 1000.0f : (float)state;
        t0 = t0 / den;
        t1 = t1 / den;
        if (want_t) {
            const size_t o = (((size_t)b * c.anchors_of_scale[s] + a) * H + py) * W + px;
            if (p.t_omask) p.t_omask[o] = state;
            if (p.t_torien) { p.t_torien[2 * o] = t0; p.t_torien[2 * o + 1] = t1; }
        }
        if (state == 0 || !p.orien[s]) continue;
        int i0, i1, j0, j1;
        float wy0, wy1, wx0, wx1;
        tap(py, 0.25f, oh, i0, i1, wy0, wy1);
        tap(px, 0.25f, ow, j0, j1, wx0, wx1);
        const float pox = bilinear_blend(pxp[i0 * ost[2] + j0], pxp[i0 * ost[2] + j1], pxp[i1 * ost[2] + j0], pxp[i1 * ost[2] + j1],
                                         wx0, wx1, wy0, wy1);
        const float poy = bilinear_blend(pyp[i0 * ost[2] + j0], pyp[i0 * ost[2] + j1], pyp[i1 * ost[2] + j0], pyp[i1 * ost[2] + j1],
                                         wx0, wx1, wy0, wy1);
        const float zx = fabsf(pox - t0), zy = fabsf(poy - t1);
        const float lx = zx < 1.0f ? 0.5f * zx * zx / 1.0f : zx - 0.5f;
        const float ly = zy < 1.0f ? 0.5f * zy * zy / 1.0f : zy - 0.5f;
        const double acc = (zx < 0.5f ? 1.0 : 0.0) + (zy < 0.5f ? 1.0 : 0.0);
        if (state < 0) {
            v[0] += (double)lx + (double)ly;
            v[2] += 1.0;
            v[4] += acc;
        } else {
            v[1] += (double)lx + (double)ly;
            v[3] += 1.0;
            v[5] += acc;
        }
    }
    block_sum<LOSS_OR_VALS, LOSS_OR_THREADS>(v, s_red);
    if (threadIdx.x == 0)
        for (int i = 0; i < LOSS_OR_VALS; ++i) part[i] = v[i];
}

// ------------------------------------------------------------------------------------------------
// reduce: one workgroup per scale; fixed-order sums of the partials, then orienmask_yolo_loss.py:122-145 and base.py:29-32
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void loss_reduce_kernel(const LossParams p) {
    __shared__ double s_v[256];
    __shared__ double s_tot[LOSS_BOX_VALS + LOSS_OR_VALS];
    const int s = blockIdx.x;
    const size_t nb = (size_t)p.B * p.box_blocks, no = (size_t)p.B * 3 * p.tiles;
    const double* bp = p.box_part + (size_t)s * nb * LOSS_BOX_VALS;
    const double* op = p.or_part + (size_t)s * no * LOSS_OR_VALS;
    for (int i = 0; i < LOSS_BOX_VALS + LOSS_OR_VALS; ++i) {
        double acc = 0.0;
        if (i < LOSS_BOX_VALS) {
            for (size_t k = threadIdx.x; k < nb; k += 256) acc += bp[k * LOSS_BOX_VALS + i];
        } else {
            for (size_t k = threadIdx.x; k < no; k += 256) acc += op[k * LOSS_OR_VALS + (i - LOSS_BOX_VALS)];
        }
        s_v[threadIdx.x] = acc;
        __syncthreads();
        for (int h = 128; h >= 1; h >>= 1) {
            if ((int)threadIdx.x < h) s_v[threadIdx.x] += s_v[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) s_tot[i] = s_v[0];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double* t = s_tot;
    const double* o = s_tot + LOSS_BOX_VALS;
    const float nB = (float)p.B;
    const float npos = (float)t[9], nneg = (float)t[10];
    const float nop = (float)o[2], non = (float)o[3];
    float term[OM_LOSS_TERMS];
    term[0] = (float)t[0] / nB;
    term[1] = (float)t[1] / 2.0f / nB;
    term[2] = (float)t[2] / nB;
    term[3] = (float)t[3] / nB;
    term[4] = (float)t[4] / nB;
    term[5] = nop > 0.0f ? (float)o[0] / nop * npos / nB : 0.0f;
    term[6] = non > 0.0f ? (float)o[1] / non * npos / nB : 0.0f;
    float* r = p.result + s * OM_LOSS_SCALE_FLOATS;
    for (int j = 0; j < OM_LOSS_TERMS; ++j) r[j] = term[j] * p.cfg.weight[s][j];
    float* m = r + OM_LOSS_TERMS;
    const float met[2 * OM_LOSS_METRICS] = {(float)t[5], npos, (float)t[6], npos, (float)t[7], nneg, (float)t[8], npos,
                                            (float)t[11], npos, (float)t[12], npos, (float)o[4], nop * 2.0f, (float)o[5], non * 2.0f};
    for (int j = 0; j < 2 * OM_LOSS_METRICS; ++j) m[j] = met[j];
}

struct LossLayout {
    size_t gts, box, orr, total;
    int box_blocks, tiles, tiles_x;
};

static bool loss_cfg_ok(const om_loss_cfg* c) {
    if (!c || c->num_scales < 1 || c->num_scales > OM_MAX_SCALES) return false;
    if (c->num_classes < 1 || c->num_classes > OM_LOSS_MAX_CLASSES) return false;
    if (c->num_anchors_total < 1 || c->num_anchors_total > OM_MAX_ANCHORS) return false;
    if (c->image_h < 4 || c->image_w < 4 || c->image_h % 4 || c->image_w % 4) return false;
    for (int s = 0; s < c->num_scales; ++s) {
        if (c->grid_h[s] < 1 || c->grid_w[s] < 1 || c->anchors_of_scale[s] < 1 || c->anchors_of_scale[s] > 3) return false;
        for (int a = 0; a < c->anchors_of_scale[s]; ++a)
            if (c->anchor_mask[s][a] < 0 || c->anchor_mask[s][a] >= c->num_anchors_total) return false;
    }
    return true;
}

static LossLayout loss_layout(const om_loss_cfg* c, int B, int N) {
    LossLayout L;
    int maxcells = 0;
    for (int s = 0; s < c->num_scales; ++s) maxcells = std::max(maxcells, c->anchors_of_scale[s] * c->grid_h[s] * c->grid_w[s]);
    L.box_blocks = (maxcells + LOSS_BOX_THREADS - 1) / LOSS_BOX_THREADS;
    L.tiles_x = (c->image_w + LOSS_TILE_W - 1) / LOSS_TILE_W;
    L.tiles = L.tiles_x * ((c->image_h + LOSS_TILE_H - 1) / LOSS_TILE_H);
    L.gts = 0;
    L.box = align_up((size_t)OM_MAX_SCALES * std::max(N, 1) * sizeof(LossGt), 256);
    L.orr = L.box + align_up((size_t)OM_MAX_SCALES * B * L.box_blocks * LOSS_BOX_VALS * sizeof(double), 256);
    L.total = L.orr + align_up((size_t)OM_MAX_SCALES * B * 3 * L.tiles * LOSS_OR_VALS * sizeof(double), 256);
    return L;
}

static int loss_run(const om_loss_cfg* cfg, const float* const* bbox, const float* const* orien, int B, const float* gt_bbox,
                    const int64_t* gt_cls, const int64_t* gt_index, const uint8_t* gt_mask, int N, float* result, void* workspace,
                    size_t ws_bytes, hipStream_t st, LossParams& p, const char* what) {
    OM_REQUIRE(loss_cfg_ok(cfg), OM_EINVAL, "%s: unsupported configuration (1..3 scales of 1..3 anchors, <= %d classes, <= 9 "
               "anchors, image sides divisible by 4)", what, OM_LOSS_MAX_CLASSES);
    OM_REQUIRE(B >= 1 && N >= 0 && N <= B * OM_LOSS_MAX_GT, OM_EINVAL, "%s: B = %d, N = %d (at most %d GTs per image)", what, B, N,
               OM_LOSS_MAX_GT);
    // N == 0 (a batch without a single GT): the GT arrays are never addressed and may be null, which is what an empty tensor hands over
    OM_REQUIRE(bbox && gt_index && workspace && result && (N == 0 || (gt_bbox && gt_cls && gt_mask)), OM_EINVAL, "%s: null pointer", what);
    for (int s = 0; s < cfg->num_scales; ++s) OM_REQUIRE(bbox[s] && (!orien || orien[s]), OM_EINVAL, "%s: null head of scale %d", what, s);
    const LossLayout L = loss_layout(cfg, B, N);
    OM_REQUIRE(ws_bytes >= L.total, OM_ENOMEM, "%s: workspace of %zu bytes, %zu needed", what, ws_bytes, L.total);
    OM_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 256 == 0, OM_EINVAL, "%s: workspace not 256-byte aligned", what);
    p.cfg = *cfg;
    for (int s = 0; s < OM_MAX_SCALES; ++s) {
        p.bbox[s] = s < cfg->num_scales ? bbox[s] : nullptr;
        p.orien[s] = (orien && s < cfg->num_scales) ? orien[s] : nullptr;
    }
    p.B = B;
    p.N = N;
    p.gt_bbox = gt_bbox;
    p.gt_cls = gt_cls;
    p.gt_index = gt_index;
    p.gt_mask = gt_mask;
    char* ws = static_cast<char*>(workspace);
    p.gts = reinterpret_cast<LossGt*>(ws + L.gts);
    p.box_part = reinterpret_cast<double*>(ws + L.box);
    p.or_part = reinterpret_cast<double*>(ws + L.orr);
    p.box_blocks = L.box_blocks;
    p.tiles = L.tiles;
    p.tiles_x = L.tiles_x;
    p.result = result;
    if (int rc = launch_zero_words(result, OM_LOSS_RESULT_FLOATS, st)) return rc;
    const int S = cfg->num_scales;
    hipLaunchKernelGGL(loss_match_kernel, dim3((std::max(N, B + 1) + 255) / 256, S), dim3(256), 0, st, p);
    OM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(loss_box_kernel, dim3(L.box_blocks, B, S), dim3(LOSS_BOX_THREADS), 0, st, p);
    OM_CHECK_HIP(hipGetLastError());
    if (p.orien[0] || p.t_omask || p.t_torien) {
        hipLaunchKernelGGL(loss_orien_kernel, dim3(L.tiles, B * 3, S), dim3(LOSS_OR_THREADS), 0, st, p);
        OM_CHECK_HIP(hipGetLastError());
    }
    return OM_OK;
}

// ------------------------------------------------------------------------------------------------
// backward: d(g * loss_sum) / d(pred_bbox, pred_orien) along the reference's autograd chain, in torch-CPU's float32 order
// (probed on torch 2.10: binary_cross_entropy_backward, sigmoid_backward, mse_loss_backward, smooth_l1_loss_backward and
// upsample_bilinear2d_backward bit for bit).  Runs after om_loss on the same inputs: the LossGt records come from its workspace,
// the counts (bbox_pos, orientation pos / neg) from its result vector.  Every gradient element is written exactly once.
// ------------------------------------------------------------------------------------------------
constexpr int LOSS_GQ = 16;                     // quarter-resolution tile side of loss_orien_grad_kernel
constexpr int LOSS_GR = 4 * LOSS_GQ + 4;        // full-resolution rows / columns its adjoint reads (2 above, 2 below)

struct LossGradParams {
    om_loss_cfg cfg;
    const float* bbox[OM_MAX_SCALES];
    const float* orien[OM_MAX_SCALES];
    float* gbbox[OM_MAX_SCALES];                // written through the heads' strides
    float* gorien[OM_MAX_SCALES];
    float sw[OM_MAX_SCALES];                    // scales_weight
    int B, N;
    const int64_t* gt_index;
    const uint8_t* gt_mask;
    const LossGt* gts;
    const float* result;
    const float* gout;                          // d(out) / d(loss_sum), device scalar
    int qtiles, qtiles_x;
};

__device__ __forceinline__ void image_range(const LossGradParams& p, int b, int& g0, int& n) {
    long long lo = p.gt_index[b], hi = p.gt_index[b + 1];
    lo = lo < 0 ? 0 : lo > p.N ? p.N : lo;
    hi = hi < lo ? lo : hi > p.N ? p.N : hi;
    g0 = (int)lo;
    n = (int)(hi - lo);
    if (n > OM_LOSS_MAX_GT) n = OM_LOSS_MAX_GT;
}

// binary_cross_entropy_backward: grad * (p - t) / max((1 - p) * p, EPSILON); sigmoid_backward: grad * (1 - p) * p
__device__ __forceinline__ float bce_grad(float d, float pr, float t) { return (d * (pr - t)) / maxf_((1.0f - pr) * pr, 1e-12f); }
__device__ __forceinline__ float sigmoid_grad(float d, float pr) { return (d * (1.0f - pr)) * pr; }

// upstream gradient of term j of scale s: (g * scales_weight[s]) * weight[s][j]  (base.py:119 then base.py:32)
__device__ __forceinline__ float term_grad(const LossGradParams& p, int s, int j) {
    return (p.gout[0] * p.sw[s]) * p.cfg.weight[s][j];
}

// box: one lane per prediction cell (b, a, gy, gx), all 5 + C channels of the cell.  grid (box_blocks, B, scales)
__global__ __launch_bounds__(LOSS_BOX_THREADS) void loss_box_grad_kernel(const LossGradParams p) {
    __shared__ float4 s_box[OM_LOSS_MAX_GT];
    __shared__ int s_key[OM_LOSS_MAX_GT];
    __shared__ int s_cls[OM_LOSS_MAX_GT];
    const int s = blockIdx.z, b = blockIdx.y;
    const om_loss_cfg& c = p.cfg;
    if (s >= c.num_scales) return;
    const int nH = c.grid_h[s], nW = c.grid_w[s], A = c.anchors_of_scale[s], C = c.num_classes;
    const int ncell = A * nH * nW;
    if ((int)blockIdx.x * LOSS_BOX_THREADS >= ncell) return;
    int g0, ng;
    image_range(p, b, g0, ng);
    const LossGt* gts = p.gts + (size_t)s * p.N + g0;
    for (int j = threadIdx.x; j < ng; j += LOSS_BOX_THREADS) {
        const LossGt& g = gts[j];
        s_box[j] = make_float4(g.gx, g.gy, g.gw, g.gh);
        s_key[j] = g.key;
        s_cls[j] = g.cls;
    }
    __syncthreads();
    const int cell = blockIdx.x * LOSS_BOX_THREADS + threadIdx.x;
    if (cell >= ncell) return;
    const int a = cell / (nH * nW), rem = cell - a * (nH * nW);
    const int gy = rem / nW, gx = rem - gy * nW;
    const int64_t* st = c.bbox_stride[s];
    const int64_t off = b * st[0] + (int64_t)a * (5 + C) * st[1] + gy * st[2] + gx * st[3];
    const float* hp = p.bbox[s] + off;
    float* gp = p.gbbox[s] + off;
    // the forward's decode, ignore mask and winner (loss_box_kernel)
    const float vx = hp[0], vy = hp[st[1]], vw = hp[2 * st[1]], vh = hp[3 * st[1]], vo = hp[4 * st[1]];
    const int ag = c.anchor_mask[s][a];
    const float sw = (float)c.image_w / (float)nW, sh = (float)c.image_h / (float)nH;
    const float sx = sigmoid_scalar_ref(vx), sy = sigmoid_scalar_ref(vy), so = sigmoid_scalar_ref(vo);
    const float x = sx + (float)gx, y = sy + (float)gy;
    const float w = expf_cr(vw) * (c.anchor_w[ag] / sw), h = expf_cr(vh) * (c.anchor_h[ag] / sh);
    const float b1x1 = x - w / 2.0f, b1y1 = y - h / 2.0f, b1x2 = x + w / 2.0f, b1y2 = y + h / 2.0f;
    const float area1 = (b1x2 - b1x1) * (b1y2 - b1y1);
    bool ignore = false;
    int win = -1, nmatch = 0;
    int cls4[4];
    for (int j = 0; j < ng; ++j) {
        const float4 g = s_box[j];
        const float b2x1 = g.x - g.z / 2.0f, b2y1 = g.y - g.w / 2.0f, b2x2 = g.x + g.z / 2.0f, b2y2 = g.y + g.w / 2.0f;
        float dx = minf_(b1x2, b2x2) - maxf_(b1x1, b2x1);
        float dy = minf_(b1y2, b2y2) - maxf_(b1y1, b2y1);
        dx = dx < 0.0f ? 0.0f : dx;
        dy = dy < 0.0f ? 0.0f : dy;
        const float inter = dx * dy;
        const float area2 = (b2x2 - b2x1) * (b2y2 - b2y1);
        const float iou = inter / ((area1 + area2) - inter);
        ignore = ignore || iou > c.obj_ignore_threshold;
        if (s_key[j] == cell) {
            win = j;
            if (nmatch < 4) cls4[nmatch] = s_cls[j];
            ++nmatch;
        }
    }
    const bool pos = win >= 0, neg = !pos && !ignore;
    const float nB = (float)p.B;
    const int64_t cs = st[1];
    // obj / noobj share loss_obj_all: its gradient is G2 / nB * pos_mask + G3 / nB * neg_mask (the ignored cells get neither)
    const float d_obj = pos ? term_grad(p, s, 2) / nB : neg ? term_grad(p, s, 3) / nB : 0.0f;
    const float g_obj = sigmoid_grad(bce_grad(d_obj, so, pos ? 1.0f : 0.0f), so);
    if (!pos) {
        gp[0] = 0.0f;
        gp[cs] = 0.0f;
        gp[2 * cs] = 0.0f;
        gp[3 * cs] = 0.0f;
        gp[4 * cs] = g_obj;
        for (int k = 0; k < C; ++k) gp[(5 + k) * cs] = 0.0f;
        return;
    }
    const LossGt& gw_ = gts[win];
    const float ps = gw_.pscale;
    const float d_xy = (term_grad(p, s, 0) / nB) * ps;                    // (bce * pos_scale).sum() / nB
    const float d_wh = ((term_grad(p, s, 1) / nB) / 2.0f) * ps;           // (mse * pos_scale).sum() / 2 / nB
    gp[0] = sigmoid_grad(bce_grad(d_xy, sx, gw_.tx), sx);
    gp[cs] = sigmoid_grad(bce_grad(d_xy, sy, gw_.ty), sy);
    gp[2 * cs] = (2.0f * (vw - gw_.tw)) * d_wh;                          // mse_loss_backward: 2 * (x - t) * grad
    gp[3 * cs] = (2.0f * (vh - gw_.th)) * d_wh;
    gp[4 * cs] = g_obj;
    const float d_cls = term_grad(p, s, 4) / nB;                         // (bce * pos_mask).sum() / nB
    const float* cp = hp + 5 * cs;
    for (int k = 0; k < C; ++k) {
        bool on = false;
        if (nmatch <= 4) {
            for (int m = 0; m < nmatch; ++m) on = on || cls4[m] == k;
        } else {
            for (int j = 0; j < ng; ++j) on = on || (s_key[j] == cell && s_cls[j] == k);
        }
        const float t = on ? c.label_on : c.label_smooth;
        const float sc = sigmoid_class_ref(cp[k * cs], k, C);
        gp[(5 + k) * cs] = sigmoid_grad(bce_grad(d_cls, sc, t), sc);
    }
}

// orientation: one workgroup per (scale, image, anchor, LOSS_GQ^2 quarter-resolution tile).  The full-resolution targets and
// d loss / d(up-sampled head) of the tile and its halo go to LDS (the forward's culled, collate-order walk); each quarter pixel
// then gathers the adjoint of the x4 bilinear up-sample from its <= 8 x 8 contributors in upsample_bilinear2d_backward's order
// (output pixels row-major, taps 00 01 10 11, each acc = fma(h * w, grad, acc)).  grid (qtiles, B * 3, scales)
__global__ __launch_bounds__(LOSS_OR_THREADS) void loss_orien_grad_kernel(const LossGradParams p) {
    __shared__ int4 s_roi[OM_LOSS_MAX_GT];
    __shared__ float4 s_geo[OM_LOSS_MAX_GT];
    __shared__ int s_idx[OM_LOSS_MAX_GT];
    __shared__ int s_n;
    __shared__ float2 s_d[LOSS_GR * LOSS_GR];
    static_assert(LOSS_GQ * LOSS_GQ == LOSS_OR_THREADS, "one lane per quarter pixel");
    const int s = blockIdx.z, b = blockIdx.y / 3, a = blockIdx.y - 3 * (blockIdx.y / 3);
    const om_loss_cfg& c = p.cfg;
    if (s >= c.num_scales || a >= c.anchors_of_scale[s]) return;
    const int H = c.image_h, W = c.image_w, oh = H / 4, ow = W / 4;
    const int qy0 = (blockIdx.x / p.qtiles_x) * LOSS_GQ, qx0 = (blockIdx.x % p.qtiles_x) * LOSS_GQ;
    const int fy0 = max(4 * qy0 - 2, 0), fy1 = min(4 * (qy0 + LOSS_GQ) + 2, H);
    const int fx0 = max(4 * qx0 - 2, 0), fx1 = min(4 * (qx0 + LOSS_GQ) + 2, W);
    const int qi = qy0 + threadIdx.x / LOSS_GQ, qj = qx0 + threadIdx.x % LOSS_GQ;
    const bool qin = qi < oh && qj < ow;
    const int64_t* ost = c.orien_stride[s];
    float* gxp = p.gorien[s] + b * ost[0] + (int64_t)(2 * a) * ost[1];
    float* gyp = gxp + ost[1];
    int g0, ng;
    image_range(p, b, g0, ng);
    const LossGt* gts = p.gts + (size_t)s * p.N + g0;
    if (threadIdx.x < 64) {         // cull in collate order: one wave, ballot + prefix
        const int lane = threadIdx.x;
        int base = 0;
        for (int j0 = 0; j0 < ng; j0 += 64) {
            const int j = j0 + lane;
            bool mine = false;
            LossGt g;
            if (j < ng) {
                g = gts[j];
                mine = g.key >= 0 && g.a == a && g.x1 < fx1 && g.x2 > fx0 && g.y1 < fy1 && g.y2 > fy0;
            }
            const unsigned long long votes = __ballot(mine);
            if (mine) {
                const int slot = base + __popcll(votes & ((1ull << lane) - 1ull));
                s_roi[slot] = make_int4(g.x1, g.x2, g.y1, g.y2);
                s_geo[slot] = make_float4(g.px, g.py, g.cw, g.ch);
                s_idx[slot] = g0 + j;
            }
            base += __popcll(votes);
        }
        if (lane == 0) s_n = base;
    }
    __syncthreads();
    const int n_inst = s_n;
    if (n_inst == 0) {              // no ROI meets the tile: the gradient is zero
        if (qin) {
            gxp[qi * ost[2] + qj] = 0.0f;
            gyp[qi * ost[2] + qj] = 0.0f;
        }
        return;
    }
    // d loss_orien_{pos,neg} / d loss_orien_all: G / nB * bbox_pos.sum() / num_orien_{pos,neg} (none when the count is 0)
    const float* r = p.result + s * OM_LOSS_SCALE_FLOATS;
    const float nB = (float)p.B, nbox = r[OM_LOSS_TERMS + 1];
    const float nop = r[OM_LOSS_TERMS + 13] / 2.0f, non = r[OM_LOSS_TERMS + 15] / 2.0f;
    const float c_pos = nop > 0.0f ? ((term_grad(p, s, 5) / nB) * nbox) / nop : 0.0f;
    const float c_neg = non > 0.0f ? ((term_grad(p, s, 6) / nB) * nbox) / non : 0.0f;
    const int ag = c.anchor_mask[s][a];
    const float haw = c.anchor_w[ag] / 2.0f, hah = c.anchor_h[ag] / 2.0f;
    const float* pxp = p.orien[s] + b * ost[0] + (int64_t)(2 * a) * ost[1];
    const float* pyp = pxp + ost[1];
    const int rh = fy1 - fy0, rw = fx1 - fx0;
    for (int k = threadIdx.x; k < rh * rw; k += LOSS_OR_THREADS) {
        const int ry = k / rw, rx = k - ry * rw;
        const int py = fy0 + ry, px = fx0 + rx;
        int state = 0;
        float t0 = 0.0f, t1 = 0.0f;
        const float fx = (float)px, fy = (float)py;
        for (int i = 0; i < n_inst; ++i) {
            const int4 roi = s_roi[i];
            if (px < roi.x || px >= roi.y || py < roi.z || py >= roi.w) continue;
            const float4 g = s_geo[i];
            const float ox = fx - g.x, oy = fy - g.y;
            if (p.gt_mask[((size_t)s_idx[i] * H + py) * W + px]) {
                state = -1;
                t0 = ox;
                t1 = oy;
            } else if (state >= 0) {
                state += 1;
                const float lx = maxf_(fabsf(ox), 1e-8f), ly = maxf_(fabsf(oy), 1e-8f);
                const float qx = maxf_(g.z / lx, 1.0f), qy = maxf_(g.w / ly, 1.0f);
                const float q = minf_(qx, qy) - 1.0f;
                const float sgx = ox > 0.0f ? 1.0f : ox < 0.0f ? -1.0f : 0.0f;
                const float sgy = oy > 0.0f ? 1.0f : oy < 0.0f ? -1.0f : 0.0f;
                t0 = t0 + (q * sgx) * lx;
                t1 = t1 + (q * sgy) * ly;
            }
        }
        float2 d = make_float2(0.0f, 0.0f);
        if (state != 0) {
            t0 = t0 / haw;
            t1 = t1 / hah;
            const float den = state < 0 ? -1.0f : (float)state;
            t0 = t0 / den;
            t1 = t1 / den;
            int i0, i1, j0, j1;
            float wy0, wy1, wx0, wx1;
            tap(py, 0.25f, oh, i0, i1, wy0, wy1);
            tap(px, 0.25f, ow, j0, j1, wx0, wx1);
            const float pox = bilinear_blend(pxp[i0 * ost[2] + j0], pxp[i0 * ost[2] + j1], pxp[i1 * ost[2] + j0],
                                             pxp[i1 * ost[2] + j1], wx0, wx1, wy0, wy1);
            const float poy = bilinear_blend(pyp[i0 * ost[2] + j0], pyp[i0 * ost[2] + j1], pyp[i1 * ost[2] + j0],
                                             pyp[i1 * ost[2] + j1], wx0, wx1, wy0, wy1);
            const float dd = state < 0 ? c_pos : c_neg;
            // smooth_l1_loss_backward, beta 1: (|x| < 1 ? x : sign(x)) * grad
            const float ex = pox - t0, ey = poy - t1;
            d.x = (fabsf(ex) < 1.0f ? ex : ex > 0.0f ? 1.0f : -1.0f) * dd;
            d.y = (fabsf(ey) < 1.0f ? ey : ey > 0.0f ? 1.0f : -1.0f) * dd;
        }
        s_d[ry * LOSS_GR + rx] = d;
    }
    __syncthreads();
    if (!qin) return;
    float ax = 0.0f, ay = 0.0f;
    const int r0 = max(4 * qi - 2, 0), r1 = min(4 * qi + 6, H), c0 = max(4 * qj - 2, 0), c1 = min(4 * qj + 6, W);
    for (int y = r0; y < r1; ++y) {
        int i0, i1;
        float wy0, wy1;
        tap(y, 0.25f, oh, i0, i1, wy0, wy1);
        if (i0 != qi && i1 != qi) continue;
        for (int x = c0; x < c1; ++x) {
            int j0, j1;
            float wx0, wx1;
            tap(x, 0.25f, ow, j0, j1, wx0, wx1);
            if (j0 != qj && j1 != qj) continue;
            const float2 d = s_d[(y - fy0) * LOSS_GR + (x - fx0)];
            if (i0 == qi && j0 == qj) { const float l = wy0 * wx0; ax = fmaf(l, d.x, ax); ay = fmaf(l, d.y, ay); }
            if (i0 == qi && j1 == qj) { const float l = wy0 * wx1; ax = fmaf(l, d.x, ax); ay = fmaf(l, d.y, ay); }
            if (i1 == qi && j0 == qj) { const float l = wy1 * wx0; ax = fmaf(l, d.x, ax); ay = fmaf(l, d.y, ay); }
            if (i1 == qi && j1 == qj) { const float l = wy1 * wx1; ax = fmaf(l, d.x, ax); ay = fmaf(l, d.y, ay); }
        }
    }
    gxp[qi * ost[2] + qj] = ax;
    gyp[qi * ost[2] + qj] = ay;
}

}  // namespace om

extern "C" {

size_t om_loss_workspace_bytes(const om_loss_cfg* cfg, int B, int N) {
    if (!om::loss_cfg_ok(cfg) || B < 1 || N < 0) return 0;
    return om::loss_layout(cfg, B, N).total;
}

int om_loss(const om_loss_cfg* cfg, const float* const* bbox, const float* const* orien, int B, const float* gt_bbox,
            const int64_t* gt_cls, const int64_t* gt_index, const uint8_t* gt_mask, int N, float* result, void* workspace,
            size_t ws_bytes, om_stream stream) {
    OM_REQUIRE(orien, OM_EINVAL, "om_loss: null orientation heads");
    om::LossParams p = {};
    p.tgt_scale = -1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = om::loss_run(cfg, bbox, orien, B, gt_bbox, gt_cls, gt_index, gt_mask, N, result, workspace, ws_bytes, st, p, "om_loss");
    if (rc != OM_OK) return rc;
    hipLaunchKernelGGL(om::loss_reduce_kernel, dim3(cfg->num_scales), dim3(256), 0, st, p);
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

int om_loss_targets(const om_loss_cfg* cfg, const float* const* bbox, int B, const float* gt_bbox, const int64_t* gt_cls,
                    const int64_t* gt_index, const uint8_t* gt_mask, int N, int scale, float* bbox_pos, float* bbox_neg,
                    float* pos_scale, float* txy, float* twh, float* tiou, float* tcls, int32_t* orien_mask, float* torien,
                    void* workspace, size_t ws_bytes, om_stream stream) {
    OM_REQUIRE(om::loss_cfg_ok(cfg), OM_EINVAL, "om_loss_targets: unsupported configuration");
    OM_REQUIRE(scale >= 0 && scale < cfg->num_scales, OM_EINVAL, "om_loss_targets: bad scale %d", scale);
    OM_REQUIRE(B >= 1 && N >= 0, OM_EINVAL, "om_loss_targets: B = %d, N = %d", B, N);
    om::LossParams p = {};
    p.tgt_scale = scale;
    p.t_pos = bbox_pos; p.t_neg = bbox_neg; p.t_pscale = pos_scale; p.t_txy = txy; p.t_twh = twh; p.t_tiou = tiou;
    p.t_tcls = tcls; p.t_omask = orien_mask; p.t_torien = torien;
    // the flag word and the (unused) sums: a result vector of their own, behind the workspace om_loss would use
    const om::LossLayout L = om::loss_layout(cfg, B, N);
    OM_REQUIRE(ws_bytes >= L.total + 512, OM_ENOMEM, "om_loss_targets: workspace of %zu bytes, %zu needed", ws_bytes, L.total + 512);
    float* res = reinterpret_cast<float*>(static_cast<char*>(workspace) + L.total);
    return om::loss_run(cfg, bbox, nullptr, B, gt_bbox, gt_cls, gt_index, gt_mask, N, res, workspace, ws_bytes,
                        static_cast<hipStream_t>(stream), p, "om_loss_targets");
}

int om_loss_backward(const om_loss_cfg* cfg, const float* const* bbox, const float* const* orien, int B, const int64_t* gt_index,
                     const uint8_t* gt_mask, int N, const float* result, const void* workspace, size_t ws_bytes,
                     const float* grad_out, const float* scales_weight, float* const* grad_bbox, float* const* grad_orien,
                     om_stream stream) {
    OM_REQUIRE(om::loss_cfg_ok(cfg), OM_EINVAL, "om_loss_backward: unsupported configuration");
    OM_REQUIRE(B >= 1 && N >= 0 && N <= B * OM_LOSS_MAX_GT, OM_EINVAL, "om_loss_backward: B = %d, N = %d", B, N);
    OM_REQUIRE(bbox && orien && grad_bbox && grad_orien && gt_index && (N == 0 || gt_mask) && result && workspace && grad_out && scales_weight,
               OM_EINVAL, "om_loss_backward: null pointer");
    const om::LossLayout L = om::loss_layout(cfg, B, N);
    OM_REQUIRE(ws_bytes >= L.total, OM_ENOMEM, "om_loss_backward: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
    om::LossGradParams p = {};
    p.cfg = *cfg;
    for (int s = 0; s < cfg->num_scales; ++s) {
        OM_REQUIRE(bbox[s] && orien[s] && grad_bbox[s] && grad_orien[s], OM_EINVAL, "om_loss_backward: null head of scale %d", s);
        p.bbox[s] = bbox[s];
        p.orien[s] = orien[s];
        p.gbbox[s] = grad_bbox[s];
        p.gorien[s] = grad_orien[s];
        p.sw[s] = scales_weight[s];
    }
    p.B = B;
    p.N = N;
    p.gt_index = gt_index;
    p.gt_mask = gt_mask;
    p.gts = reinterpret_cast<const om::LossGt*>(static_cast<const char*>(workspace) + L.gts);
    p.result = result;
    p.gout = grad_out;
    p.qtiles_x = (cfg->image_w / 4 + om::LOSS_GQ - 1) / om::LOSS_GQ;
    p.qtiles = p.qtiles_x * ((cfg->image_h / 4 + om::LOSS_GQ - 1) / om::LOSS_GQ);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int S = cfg->num_scales;
    hipLaunchKernelGGL(om::loss_box_grad_kernel, dim3(L.box_blocks, B, S), dim3(om::LOSS_BOX_THREADS), 0, st, p);
    OM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(om::loss_orien_grad_kernel, dim3(p.qtiles, B * 3, S), dim3(om::LOSS_OR_THREADS), 0, st, p);
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

}  // extern "C"
