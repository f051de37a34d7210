// Training / validation augmentation of the reference's data loader: COCOTransform (data/transform.py:65-441) and collate
// (data/collate.py:13-30), the pixel half.  orienmask_amd/augment.py draws every random number on the host, in the reference's
// order, and hands over one om_aug_sample per image; these kernels then produce the collated batch on the device:
//   aug_gray_partial / aug_gray_final  the grey mean adjust_contrast takes over the FULL source (cv2 RGB2GRAY .mean()), with the
//                                      jitter ops that precede contrast applied per pixel.  Fixed-order reduction: double partials
//                                      per workgroup, then one fixed tree per image -- no atomics, bit-identical run to run.
//   aug_image_kernel                   one pass over the [B,3,H,W] output: flips undone, pad colour, cv2 INTER_LINEAR into the
//                                      crop window (INTER_AREA's 2x2 mean on an exact 2x downscale) with the jitter chain on each
//                                      tap, Normalize.  No jittered or resized intermediate is materialised.
//   aug_mask_kernel                    [N,H,W] bool: cv2 INTER_NEAREST from the row-packed bits, pad 0, flips, written at the GT's
//                                      ToTensor-permuted index, 16 bytes per thread.
// cv2's float code paths restated here (DESIGN.md section "Training augmentation"): resize.cpp (linear coefficients, resizeNN),
// color_hsv (RGB2HSV_f / HSV2RGB_f), color_rgb (RGB2Gray<float>).  Built with -ffp-contract=off: every product is rounded as
// the float32 code it restates rounds it.
#include "om_common.h"

namespace om {

constexpr int AUG_THREADS = 256;
constexpr int AUG_GRAY_BLOCKS = 256;        // workgroups per image of the grey-mean reduction (fixed: the sum order depends on it)
constexpr int AUG_MASK_BYTES = 16;          // output bytes per thread of the mask kernel
constexpr float AUG_FLT_EPSILON = 1.19209290e-07f;

struct AugParams {
    const om_aug_sample* S;
    const void* images;
    const uint8_t* masks;
    const int32_t* gt_table;
    float* out_image;
    uint8_t* out_mask;
    double* partial;
    float* gray_mean;             // null when no image has contrast
    int n_images, n_gt, out_h, out_w, mask_vec;
    float mean[3], stdv[3];
};

__device__ __forceinline__ float clip255(float v) { return fminf(fmaxf(v, 0.f), 255.f); }

// cv2 RGB2Gray<float>, RGB order: R * 0.299 + G * 0.587 + B * 0.114, summed left to right
__device__ __forceinline__ float gray_of(float r, float g, float b) { return r * 0.299f + g * 0.587f + b * 0.114f; }

// cv2 RGB2HSV_f, hrange 360 (hscale 1): H in degrees, S in [0,1], V unscaled
__device__ __forceinline__ void rgb2hsv(float r, float g, float b, float& h, float& s, float& v) {
    float vmin = r;
    v = r;
    if (v < g) v = g;
    if (v < b) v = b;
    if (vmin > g) vmin = g;
    if (vmin > b) vmin = b;
    float diff = v - vmin;
    s = diff / (fabsf(v) + AUG_FLT_EPSILON);
    diff = (float)(60.0 / (double)(diff + AUG_FLT_EPSILON));
    if (v == r) h = (g - b) * diff;
    else if (v == g) h = (b - r) * diff + 120.f;
    else h = (r - g) * diff + 240.f;
    if (h < 0.f) h += 360.f;
}

// cv2 HSV2RGB_f, hscale 6/360, its sector table
__device__ __forceinline__ void hsv2rgb(float h, float s, float v, float& r, float& g, float& b) {
    if (s == 0.f) { r = g = b = v; return; }
    h *= 6.f / 360.f;
    if (h < 0.f) { do h += 6.f; while (h < 0.f); }
    else if (h >= 6.f) { do h -= 6.f; while (h >= 6.f); }
    int sector = (int)floorf(h);
    h -= (float)sector;
    if ((unsigned)sector >= 6u) { sector = 0; h = 0.f; }
    float tab[4];
    tab[0] = v;
    tab[1] = v * (1.f - s);
    tab[2] = v * (1.f - s * h);
    tab[3] = v * (1.f - s * (1.f - h));
    switch (sector) {       // cv2's sector_data[sector] = {b, g, r} indices into tab
    case 0: b = tab[1]; g = tab[3]; r = tab[0]; break;
    case 1: b = tab[1]; g = tab[0]; r = tab[2]; break;
    case 2: b = tab[3]; g = tab[0]; r = tab[1]; break;
    case 3: b = tab[0]; g = tab[2]; r = tab[1]; break;
    case 4: b = tab[0]; g = tab[1]; r = tab[3]; break;
    default: b = tab[2]; g = tab[1]; r = tab[0]; break;
    }
}

// ops [0, n) of the image's chain on one pixel (adjust_brightness / _contrast / _saturation / _hue, float32 as numpy runs them)
__device__ __forceinline__ void apply_ops(const om_aug_sample& s, int n, float mean_fb_contrast, float& r, float& g, float& b) {
    for (int k = 0; k < n; ++k) {
        const float fa = s.fa[k], fb = s.fb[k];
        switch (s.op[k]) {
        case OM_AUG_BRIGHTNESS:
            r = clip255(r * fa); g = clip255(g * fa); b = clip255(b * fa);
            break;
        case OM_AUG_CONTRAST:
            r = clip255(r * fa + mean_fb_contrast); g = clip255(g * fa + mean_fb_contrast); b = clip255(b * fa + mean_fb_contrast);
            break;
        case OM_AUG_SATURATION: {
            const float gy = gray_of(r, g, b) * fb;
            r = clip255(r * fa + gy); g = clip255(g * fa + gy); b = clip255(b * fa + gy);
            break;
        }
        default: {      // OM_AUG_HUE: the reference clips the shifted hue to [0, 360] (no wrap) and does not clip the result
            float h, sat, val;
            rgb2hsv(r, g, b, h, sat, val);
            h = fminf(fmaxf(h + fb, 0.f), 360.f);
            hsv2rgb(h, sat, val, r, g, b);
            break;
        }
        }
    }
}

__device__ __forceinline__ int contrast_pos(const om_aug_sample& s) {
    for (int k = 0; k < s.n_ops; ++k)
        if (s.op[k] == OM_AUG_CONTRAST) return k;
    return -1;
}

template <typename T>
__device__ __forceinline__ void load_rgb(const T* p, float& r, float& g, float& b) {
    r = (float)p[0]; g = (float)p[1]; b = (float)p[2];
}

// cv2 resize.cpp, INTER_LINEAR coefficients: fx = (float)((dx + 0.5) * scale - 0.5), sx = floor, clamped at the window's edges
__device__ __forceinline__ void linear_coord(int d, double scale, int n, int& s0, int& s1, float& w1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int sx = (int)floorf(f);
    f -= (float)sx;
    if (sx < 0) { sx = 0; f = 0.f; }
    if (sx >= n - 1) { sx = n - 1; f = 0.f; }
    s0 = sx;
    s1 = sx + 1 < n ? sx + 1 : n - 1;
    w1 = f;
}

template <typename T>
__global__ __launch_bounds__(AUG_THREADS) void aug_gray_partial(const AugParams p) {
    const int img = blockIdx.y;
    const om_aug_sample& s = p.S[img];
    const int kc = contrast_pos(s);
    if (kc < 0) return;
    const long long hw = (long long)s.src_h * s.src_w;
    const long long chunk = (hw + AUG_GRAY_BLOCKS - 1) / AUG_GRAY_BLOCKS;
    const long long beg = chunk * blockIdx.x;
    const long long end = beg + chunk < hw ? beg + chunk : hw;
    const T* src = static_cast<const T*>(p.images) + s.image_off;
    double acc = 0.0;
    for (long long i = beg + threadIdx.x; i < end; i += AUG_THREADS) {
        float r, g, b;
        load_rgb(src + 3 * i, r, g, b);
        apply_ops(s, kc, 0.f, r, g, b);         // only brightness / saturation / hue can precede the first contrast
        acc += (double)gray_of(r, g, b);
    }
    __shared__ double red[AUG_THREADS];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = AUG_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.partial[(size_t)img * AUG_GRAY_BLOCKS + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(AUG_GRAY_BLOCKS) void aug_gray_final(const AugParams p) {
    const int img = blockIdx.x;
    const om_aug_sample& s = p.S[img];
    if (contrast_pos(s) < 0) return;
    __shared__ double red[AUG_GRAY_BLOCKS];
    red[threadIdx.x] = p.partial[(size_t)img * AUG_GRAY_BLOCKS + threadIdx.x];
    __syncthreads();
    for (int w = AUG_GRAY_BLOCKS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.gray_mean[img] = (float)(red[0] / ((double)s.src_h * (double)s.src_w));
}

template <typename T>
__device__ __forceinline__ void tap(const T* src, int w, int y, int x, const om_aug_sample& s, float mfb, float& r, float& g,
                                    float& b) {
    load_rgb(src + ((size_t)y * w + x) * 3, r, g, b);
    apply_ops(s, s.n_ops, mfb, r, g, b);
}

template <typename T>
__global__ __launch_bounds__(AUG_THREADS) void aug_image_kernel(const AugParams p) {
    const int img = blockIdx.y;
    const int plane = p.out_h * p.out_w;
    const int idx = blockIdx.x * AUG_THREADS + threadIdx.x;
    if (idx >= plane) return;
    const om_aug_sample& s = p.S[img];
    const int y = idx / p.out_w, x = idx - (idx / p.out_w) * p.out_w;
    const int yy = (s.vflip ? p.out_h - 1 - y : y) - s.pad_top;
    const int xx = (s.hflip ? p.out_w - 1 - x : x) - s.pad_left;
    float o[3];
    if ((unsigned)yy >= (unsigned)s.nh || (unsigned)xx >= (unsigned)s.nw) {
        o[0] = s.pad_value[0]; o[1] = s.pad_value[1]; o[2] = s.pad_value[2];
    } else {
        float mfb = 0.f;
        if (p.gray_mean) {
            const int kc = contrast_pos(s);
            if (kc >= 0) mfb = p.gray_mean[img] * s.fb[kc];
        }
        const T* src = static_cast<const T*>(p.images) + s.image_off;
        float r00, g00, b00, r01, g01, b01, r10, g10, b10, r11, g11, b11;
        if (s.area2x) {     // cv2 takes INTER_AREA's fast path for an exact 2x downscale: (S0[x] + S0[x+1] + S1[x] + S1[x+1]) * 0.25
            const int sy = s.crop_top + 2 * yy, sx = s.crop_left + 2 * xx;
            tap(src, s.src_w, sy, sx, s, mfb, r00, g00, b00);
            tap(src, s.src_w, sy, sx + 1, s, mfb, r01, g01, b01);
            tap(src, s.src_w, sy + 1, sx, s, mfb, r10, g10, b10);
            tap(src, s.src_w, sy + 1, sx + 1, s, mfb, r11, g11, b11);
            o[0] = (r00 + r01 + r10 + r11) * 0.25f;
            o[1] = (g00 + g01 + g10 + g11) * 0.25f;
            o[2] = (b00 + b01 + b10 + b11) * 0.25f;
        } else {
            int y0, y1, x0, x1;
            float fy, fx;
            linear_coord(yy, s.scale_y, s.crop_h, y0, y1, fy);
            linear_coord(xx, s.scale_x, s.crop_w, x0, x1, fx);
            y0 += s.crop_top; y1 += s.crop_top; x0 += s.crop_left; x1 += s.crop_left;
            tap(src, s.src_w, y0, x0, s, mfb, r00, g00, b00);
            tap(src, s.src_w, y0, x1, s, mfb, r01, g01, b01);
            tap(src, s.src_w, y1, x0, s, mfb, r10, g10, b10);
            tap(src, s.src_w, y1, x1, s, mfb, r11, g11, b11);
            const float ax0 = 1.f - fx, ay0 = 1.f - fy;
            // horizontal pass per row, then the vertical blend (cv2 HResizeLinear, VResizeLinear)
            o[0] = (r00 * ax0 + r01 * fx) * ay0 + (r10 * ax0 + r11 * fx) * fy;
            o[1] = (g00 * ax0 + g01 * fx) * ay0 + (g10 * ax0 + g11 * fx) * fy;
            o[2] = (b00 * ax0 + b01 * fx) * ay0 + (b10 * ax0 + b11 * fx) * fy;
        }
    }
    float* out = p.out_image + (size_t)img * 3 * plane + idx;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(size_t)c * plane] = (o[c] - p.mean[c]) / p.stdv[c];
}

__global__ __launch_bounds__(AUG_THREADS) void aug_mask_kernel(const AugParams p) {
    const int o = blockIdx.y;
    const int plane = p.out_h * p.out_w;
    const int base = (blockIdx.x * AUG_THREADS + threadIdx.x) * AUG_MASK_BYTES;
    if (base >= plane) return;
    const int src_gt = p.gt_table[2 * o], img = p.gt_table[2 * o + 1];
    const om_aug_sample& s = p.S[img];
    const int rowb = (s.src_w + 7) >> 3;
    const uint8_t* bits = p.masks + s.mask_off + (size_t)(src_gt - s.gt_first) * s.src_h * rowb;
    uint8_t v[AUG_MASK_BYTES];
#pragma unroll
    for (int k = 0; k < AUG_MASK_BYTES; ++k) {
        const int idx = base + k;
        const int y = idx / p.out_w, x = idx - (idx / p.out_w) * p.out_w;
        const int yy = (s.vflip ? p.out_h - 1 - y : y) - s.pad_top;
        const int xx = (s.hflip ? p.out_w - 1 - x : x) - s.pad_left;
        uint8_t bit = 0;
        if (idx < plane && (unsigned)yy < (unsigned)s.nh && (unsigned)xx < (unsigned)s.nw) {
            // cv2 resizeNN: min(floor(d * ifx), n - 1) in double, ifx = 1 / ((double)nw / crop_w)
            int sy = (int)floor((double)yy * s.scale_y);
            int sx = (int)floor((double)xx * s.scale_x);
            sy = (sy < s.crop_h - 1 ? sy : s.crop_h - 1) + s.crop_top;
            sx = (sx < s.crop_w - 1 ? sx : s.crop_w - 1) + s.crop_left;
            bit = (bits[(size_t)sy * rowb + (sx >> 3)] >> (7 - (sx & 7))) & 1;
        }
        v[k] = bit;
    }
    uint8_t* out = p.out_mask + (size_t)o * plane + base;
    if (p.mask_vec) {       // plane % 16 == 0: every thread's 16 bytes are aligned and inside the plane
        uint4 w;
        w.x = v[0] | (v[1] << 8) | (v[2] << 16) | ((uint32_t)v[3] << 24);
        w.y = v[4] | (v[5] << 8) | (v[6] << 16) | ((uint32_t)v[7] << 24);
        w.z = v[8] | (v[9] << 8) | (v[10] << 16) | ((uint32_t)v[11] << 24);
        w.w = v[12] | (v[13] << 8) | (v[14] << 16) | ((uint32_t)v[15] << 24);
        *reinterpret_cast<uint4*>(out) = w;
    } else {
        for (int k = 0; k < AUG_MASK_BYTES && base + k < plane; ++k) out[k] = v[k];
    }
}

}  // namespace om

extern "C" {

size_t om_augment_workspace_bytes(int n_images) {
    if (n_images <= 0) return 0;
    return om::align_up((size_t)n_images * om::AUG_GRAY_BLOCKS * sizeof(double), 256) + om::align_up((size_t)n_images * sizeof(float), 256);
}

int om_augment(const om_aug_sample* samples, int n_images, const void* images, int images_u8, const float* mean3,
               const float* std3, int out_h, int out_w, float* out_image, const uint8_t* masks, const int32_t* gt_table, int n_gt,
               uint8_t* out_mask, int any_contrast, void* workspace, size_t ws_bytes, om_stream stream) {
    OM_REQUIRE(samples && images && mean3 && std3 && out_image, OM_EINVAL, "om_augment: null argument");
    OM_REQUIRE(n_images > 0 && n_images <= 65535 && out_h > 0 && out_w > 0 && (long long)out_h * out_w < (1LL << 30), OM_EINVAL,
               "om_augment: bad shape (%d images of %dx%d)", n_images, out_h, out_w);
    OM_REQUIRE(n_gt >= 0 && n_gt <= 65535, OM_EINVAL, "om_augment: %d GTs (at most 65535 per batch)", n_gt);
    OM_REQUIRE(n_gt == 0 || (masks && gt_table && out_mask), OM_EINVAL, "om_augment: GTs without mask buffers");
    OM_REQUIRE(!any_contrast || (workspace && ws_bytes >= om_augment_workspace_bytes(n_images)), OM_ENOMEM,
               "om_augment: workspace of %zu bytes, %zu needed", ws_bytes, om_augment_workspace_bytes(n_images));
    om::AugParams p;
    p.S = samples; p.images = images; p.masks = masks; p.gt_table = gt_table; p.out_image = out_image; p.out_mask = out_mask;
    p.n_images = n_images; p.n_gt = n_gt; p.out_h = out_h; p.out_w = out_w;
    const int plane = out_h * out_w;
    p.mask_vec = plane % om::AUG_MASK_BYTES == 0 && (reinterpret_cast<uintptr_t>(out_mask) % 16) == 0;
    for (int c = 0; c < 3; ++c) { p.mean[c] = mean3[c]; p.stdv[c] = std3[c]; }
    p.partial = nullptr; p.gray_mean = nullptr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (any_contrast) {
        p.partial = static_cast<double*>(workspace);
        p.gray_mean = reinterpret_cast<float*>(static_cast<char*>(workspace) +
                                               om::align_up((size_t)n_images * om::AUG_GRAY_BLOCKS * sizeof(double), 256));
        if (images_u8)
            hipLaunchKernelGGL(om::aug_gray_partial<uint8_t>, dim3(om::AUG_GRAY_BLOCKS, n_images), dim3(om::AUG_THREADS), 0, st, p);
        else
            hipLaunchKernelGGL(om::aug_gray_partial<float>, dim3(om::AUG_GRAY_BLOCKS, n_images), dim3(om::AUG_THREADS), 0, st, p);
        OM_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(om::aug_gray_final, dim3(n_images), dim3(om::AUG_GRAY_BLOCKS), 0, st, p);
        OM_CHECK_HIP(hipGetLastError());
    }
    const dim3 grid_img((unsigned)((plane + om::AUG_THREADS - 1) / om::AUG_THREADS), n_images);
    if (images_u8)
        hipLaunchKernelGGL(om::aug_image_kernel<uint8_t>, grid_img, dim3(om::AUG_THREADS), 0, st, p);
    else
        hipLaunchKernelGGL(om::aug_image_kernel<float>, grid_img, dim3(om::AUG_THREADS), 0, st, p);
    OM_CHECK_HIP(hipGetLastError());
    if (n_gt > 0) {
        const int per_block = om::AUG_THREADS * om::AUG_MASK_BYTES;
        hipLaunchKernelGGL(om::aug_mask_kernel, dim3((unsigned)((plane + per_block - 1) / per_block), n_gt), dim3(om::AUG_THREADS), 0,
                           st, p);
        OM_CHECK_HIP(hipGetLastError());
    }
    return OM_OK;
}

}  // extern "C"
