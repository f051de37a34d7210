// Input side of the path: the reference's GPU preprocessing
//   FastCOCOTransform.__call__: [n,h,w,c] -> permute(0,3,1,2) -> Resize (F.interpolate bilinear,
//   align_corners=False) -> Normalize ((x - mean) / std)          /root/reference/data/transform.py:444-510
//   pad(image, 32, 0): centred zero padding to a multiple of 32   /root/reference/infer.py:21-32
// fused into ONE kernel that reads the HWC image once and writes the padded NCHW network input once
// (the reference runs permute+contiguous, interpolate, sub_, div_, F.pad: five passes over the image).
//
// Bit-exactness: the source index is fmaf(scale, dst + 0.5, -0.5) and the taps are combined as
// fmaf(row(y0), wy0, row(y1) * wy1) with row(y) = fmaf(v[x0], wx0, v[x1] * wx1) -- the placement torch's
// CPU kernel compiles to (found by search, see oracle/orienmask_ref.py); this file is built with
// -ffp-contract=off so nothing else fuses.  Division by std is IEEE.
//
// torch-CPU takes another kernel when the resized height + width is at most 128 (its channels-last loop, which it prefers for
// small outputs): the four weights h_i * w_j are rounded first and the taps summed left to right,
// fmaf(v11, w11, fmaf(v10, w10, fmaf(v00, w00, v01 * w01))).  A 7 x 7 image resized to 5 x 9 showed the difference
// (tests/test_geometry_sweep.py); preprocess_kernel follows both.  torch also takes that loop at EVERY size when it runs on one
// thread and the image has 3 channels: the kernel follows torch multi-threaded, as the reference runs and as the oracle
// (oracle/orienmask_ref.py) evaluates it.
#include "om_common.h"
#include "bilinear.h"

namespace om {

struct PreParams {
    const float* in;     // [N,h,w,3]
    float* out;          // [N,3,out_h,out_w]
    int N, h, w, rh, rw, out_h, out_w, pad_top, pad_left;
    int small_out;       // rh + rw <= BILINEAR_SMALL_OUT: torch-CPU blends with another kernel (bilinear.h)
    float mean[3], stdv[3], pad_value, scale_h, scale_w;
};

__device__ __forceinline__ void bilinear_tap(int d, float scale, int n_in, int& i0, int& i1, float& w0, float& w1) {
    float src = fmaf(scale, (float)d + 0.5f, -0.5f);
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    if (i0 > n_in - 1) i0 = n_in - 1;
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    w1 = src - (float)i0;
    w0 = 1.0f - w1;
}

__global__ __launch_bounds__(256) void preprocess_kernel(const PreParams p) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)p.N * p.out_h * p.out_w;
    if (idx >= total) return;
    const int x = (int)(idx % p.out_w);
    const long long r = idx / p.out_w;
    const int y = (int)(r % p.out_h);
    const int n = (int)(r / p.out_h);
    const size_t plane = (size_t)p.out_h * p.out_w;
    float* o = p.out + (size_t)n * 3 * plane + (size_t)y * p.out_w + x;
    const int ry = y - p.pad_top, rx = x - p.pad_left;
    if ((unsigned)ry >= (unsigned)p.rh || (unsigned)rx >= (unsigned)p.rw) {
        o[0] = p.pad_value; o[plane] = p.pad_value; o[2 * plane] = p.pad_value;
        return;
    }
    int y0, y1, x0, x1;
    float wy0, wy1, wx0, wx1;
    bilinear_tap(ry, p.scale_h, p.h, y0, y1, wy0, wy1);
    bilinear_tap(rx, p.scale_w, p.w, x0, x1, wx0, wx1);
    const float* img = p.in + (size_t)n * p.h * p.w * 3;
    const float* p00 = img + ((size_t)y0 * p.w + x0) * 3;
    const float* p01 = img + ((size_t)y0 * p.w + x1) * 3;
    const float* p10 = img + ((size_t)y1 * p.w + x0) * 3;
    const float* p11 = img + ((size_t)y1 * p.w + x1) * 3;
    if (p.small_out) {
        // torch-CPU's kernel for outputs with height + width <= 128: four weights h_i * w_j, summed left to right
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = bilinear_blend_small(p00[c], p01[c], p10[c], p11[c], wx0, wx1, wy0, wy1);
            o[c * plane] = (v - p.mean[c]) / p.stdv[c];
        }
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = fmaf(p00[c], wx0, p01[c] * wx1);
        const float bot = fmaf(p10[c], wx0, p11[c] * wx1);
        const float v = fmaf(top, wy0, bot * wy1);
        o[c * plane] = (v - p.mean[c]) / p.stdv[c];
    }
}

// ---- the batched form: OM_PRE_BATCH images of their own sizes and element types per launch -----------------------------------
// One table entry per image, passed by value (the kernel argument block: no device table, no copy); blockIdx.y is the image, so
// the entry is read with scalar loads and the uint8 / float32 and RGB / BGR decisions are uniform over a workgroup.  A lane
// owns VEC consecutive output pixels of one row in all three planes: VEC = 4 stores 16 bytes per plane, 1 KiB per wave and
// instruction (out_w a multiple of 4 and a 16-byte aligned output); VEC = 1 is the form for every other width.
//
// The arithmetic is preprocess_kernel's, operation for operation, and uint8 -> float32 is exact: the result has the bits
// preprocess_kernel gives for float32(image) in RGB order.
//
// Reads: the two taps of a row are neighbouring pixels (x1 = x0 + 1) or the same one (x0 = w - 1).  Of a uint8 row the six
// bytes of two neighbours are read as 4 + 2 bytes at the pixel's own (any) byte address, the three bytes of a single one byte
// by byte: nothing outside [image, image + h * w * 3) is touched, wherever the image starts and whatever lies behind it.
struct PreImg {
    const void* src;     // [h,w,3] uint8 or float32
    int h, w, rh, rw, pad_top, pad_left, flags;
    int small_out;       // as PreParams.small_out, of this image's rh + rw
    float scale_h, scale_w;
};

struct PreBatch {
    PreImg img[OM_PRE_BATCH];
    float* out;          // plane set of the group's first image
    int n, out_h, out_w;
    float mean[3], stdv[3], pad_value;
};

struct TapPair { float a0, a1, a2, b0, b1, b2; };            // channels 0..2 of the pixel at x0 (a) and at x1 (b)

__device__ __forceinline__ TapPair load_pair(const uint8_t* p, bool two) {
    TapPair r;
    if (two) {
        uint32_t lo;
        uint16_t hi;
        __builtin_memcpy(&lo, p, 4);                         // alignment 1: the compiler picks the widest load the target allows
        __builtin_memcpy(&hi, p + 4, 2);
        r.a0 = (float)(lo & 0xffu); r.a1 = (float)((lo >> 8) & 0xffu); r.a2 = (float)((lo >> 16) & 0xffu);
        r.b0 = (float)(lo >> 24); r.b1 = (float)(hi & 0xffu); r.b2 = (float)(hi >> 8);
    } else {
        r.a0 = r.b0 = (float)p[0]; r.a1 = r.b1 = (float)p[1]; r.a2 = r.b2 = (float)p[2];
    }
    return r;
}

__device__ __forceinline__ TapPair load_pair(const float* p, bool two) {
    const float* p1 = p + (two ? 3 : 0);
    TapPair r;
    r.a0 = p[0]; r.a1 = p[1]; r.a2 = p[2]; r.b0 = p1[0]; r.b1 = p1[1]; r.b2 = p1[2];
    return r;
}

// one output pixel inside the resized image: v[c] for the three OUTPUT channels
template <typename T>
__device__ __forceinline__ void pre_pixel(const PreBatch& bt, const PreImg& q, int y0, int y1, float wy0, float wy1, int rx,
                                          float v[3]) {
    int x0, x1;
    float wx0, wx1;
    bilinear_tap(rx, q.scale_w, q.w, x0, x1, wx0, wx1);
    const T* img = static_cast<const T*>(q.src);
    TapPair t = load_pair(img + ((size_t)y0 * q.w + x0) * 3, x1 != x0);
    TapPair u = load_pair(img + ((size_t)y1 * q.w + x0) * 3, x1 != x0);
    if (q.flags & OM_PRE_BGR) {                               // output channel c reads source channel 2 - c
        float s;
        s = t.a0; t.a0 = t.a2; t.a2 = s; s = t.b0; t.b0 = t.b2; t.b2 = s;
        s = u.a0; u.a0 = u.a2; u.a2 = s; s = u.b0; u.b0 = u.b2; u.b2 = s;
    }
    const float a00[3] = {t.a0, t.a1, t.a2}, a01[3] = {t.b0, t.b1, t.b2}, a10[3] = {u.a0, u.a1, u.a2}, a11[3] = {u.b0, u.b1, u.b2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t00 = a00[c], t01 = a01[c], t10 = a10[c], t11 = a11[c];
        float r;
        if (q.small_out) {
            r = bilinear_blend_small(t00, t01, t10, t11, wx0, wx1, wy0, wy1);
        } else {
            const float top = fmaf(t00, wx0, t01 * wx1);
            const float bot = fmaf(t10, wx0, t11 * wx1);
            r = fmaf(top, wy0, bot * wy1);
        }
        v[c] = (r - bt.mean[c]) / bt.stdv[c];
    }
}

template <int VEC>
__global__ __launch_bounds__(256) void preprocess_batch_kernel(const PreBatch bt) {
    const PreImg& q = bt.img[blockIdx.y];
    const int per_row = bt.out_w / VEC;
    const int item = (int)blockIdx.x * 256 + (int)threadIdx.x;          // out_h * out_w < 2^31 (the entry)
    if (item >= bt.out_h * per_row) return;
    const int y = item / per_row, x = (item - y * per_row) * VEC;
    const size_t plane = (size_t)bt.out_h * bt.out_w;
    float* o = bt.out + (size_t)blockIdx.y * 3 * plane + (size_t)y * bt.out_w + x;
    const int ry = y - q.pad_top;
    const bool row_in = (unsigned)ry < (unsigned)q.rh;
    int y0 = 0, y1 = 0;
    float wy0 = 0.f, wy1 = 0.f;
    if (row_in) bilinear_tap(ry, q.scale_h, q.h, y0, y1, wy0, wy1);
    const bool u8 = (q.flags & OM_PRE_U8) != 0;
    float r[3][VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const int rx = x + e - q.pad_left;
        float v[3] = {bt.pad_value, bt.pad_value, bt.pad_value};
        if (row_in && (unsigned)rx < (unsigned)q.rw) {
            if (u8) pre_pixel<uint8_t>(bt, q, y0, y1, wy0, wy1, rx, v);
            else pre_pixel<float>(bt, q, y0, y1, wy0, wy1, rx, v);
        }
        r[0][e] = v[0]; r[1][e] = v[1]; r[2][e] = v[2];
    }
    if constexpr (VEC == 4) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<float4*>(o + c * plane) = make_float4(r[c][0], r[c][1], r[c][2], r[c][3]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[c * plane + e] = r[c][e];
    }
}

__global__ __launch_bounds__(256) void pad_nchw_kernel(const float* __restrict__ in, float* __restrict__ out, long long planes,
                                                       int h, int w, int out_h, int out_w, int pad_top, int pad_left,
                                                       float pad_value) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= planes * out_h * out_w) return;
    const int x = (int)(idx % out_w);
    const long long r = idx / out_w;
    const int y = (int)(r % out_h);
    const long long pl = r / out_h;
    const int sy = y - pad_top, sx = x - pad_left;
    float v = pad_value;
    if ((unsigned)sy < (unsigned)h && (unsigned)sx < (unsigned)w) v = in[(pl * h + sy) * w + sx];
    out[idx] = v;
}

}  // namespace om

extern "C" {

int om_preprocess(const float* in_nhwc, int N, int h, int w, int resize_h, int resize_w, const float* mean3,
                  const float* std3, int pad_top, int pad_left, int out_h, int out_w, float pad_value, float* out_nchw,
                  om_stream stream) {
    OM_REQUIRE(in_nhwc && out_nchw && mean3 && std3, OM_EINVAL, "om_preprocess: null argument");
    OM_REQUIRE(N > 0 && h > 0 && w > 0 && resize_h > 0 && resize_w > 0, OM_EINVAL, "om_preprocess: bad shape");
    OM_REQUIRE(pad_top >= 0 && pad_left >= 0 && pad_top + resize_h <= out_h && pad_left + resize_w <= out_w, OM_EINVAL,
               "om_preprocess: the resized image (%dx%d at +%d,+%d) does not fit the output %dx%d", resize_h, resize_w,
               pad_top, pad_left, out_h, out_w);
    om::PreParams p;
    p.in = in_nhwc; p.out = out_nchw;
    p.N = N; p.h = h; p.w = w; p.rh = resize_h; p.rw = resize_w; p.out_h = out_h; p.out_w = out_w;
    p.pad_top = pad_top; p.pad_left = pad_left; p.pad_value = pad_value;
    for (int c = 0; c < 3; ++c) { p.mean[c] = mean3[c]; p.stdv[c] = std3[c]; }
    p.scale_h = (float)h / (float)resize_h;      // area_pixel_compute_scale with size= given
    p.scale_w = (float)w / (float)resize_w;
    p.small_out = resize_h + resize_w <= om::BILINEAR_SMALL_OUT ? 1 : 0;
    const long long total = (long long)N * out_h * out_w;
    hipLaunchKernelGGL(om::preprocess_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), p);
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

int om_preprocess_batch(const void* const* images, const int32_t* geom, int n, const float* mean3, const float* std3,
                        int out_h, int out_w, float pad_value, float* out_nchw, om_stream stream) {
    OM_REQUIRE(images && geom && mean3 && std3 && out_nchw, OM_EINVAL, "om_preprocess_batch: null argument");
    OM_REQUIRE(n > 0, OM_EINVAL, "om_preprocess_batch: n = %d images", n);
    OM_REQUIRE(out_h > 0 && out_w > 0 && (long long)out_h * out_w < (1ll << 31), OM_EINVAL,
               "om_preprocess_batch: bad output size %dx%d", out_h, out_w);
    OM_REQUIRE(reinterpret_cast<uintptr_t>(out_nchw) % 4 == 0, OM_EINVAL, "om_preprocess_batch: out_nchw not 4-byte aligned");
    for (int i = 0; i < n; ++i) {                             // every row before the first launch: a refused call writes nothing
        const int32_t* g = geom + 8 * (size_t)i;
        OM_REQUIRE(images[i], OM_EINVAL, "om_preprocess_batch: image %d: null pointer", i);
        OM_REQUIRE((g[6] & ~(OM_PRE_U8 | OM_PRE_BGR)) == 0 && g[7] == 0, OM_EINVAL,
                   "om_preprocess_batch: image %d: unknown flag bits (flags 0x%x, reserved %d)", i, (unsigned)g[6], g[7]);
        OM_REQUIRE(g[0] > 0 && g[1] > 0 && g[2] > 0 && g[3] > 0, OM_EINVAL,
                   "om_preprocess_batch: image %d: bad shape (%dx%d resized to %dx%d)", i, g[0], g[1], g[2], g[3]);
        OM_REQUIRE(g[4] >= 0 && g[5] >= 0 && (long long)g[4] + g[2] <= out_h && (long long)g[5] + g[3] <= out_w, OM_EINVAL,
                   "om_preprocess_batch: image %d: the resized image (%dx%d at +%d,+%d) does not fit the output %dx%d", i, g[2],
                   g[3], g[4], g[5], out_h, out_w);
        OM_REQUIRE((g[6] & OM_PRE_U8) || reinterpret_cast<uintptr_t>(images[i]) % 4 == 0, OM_EINVAL,
                   "om_preprocess_batch: image %d: a float32 image must be 4-byte aligned", i);
    }
    const bool vec = out_w % 4 == 0 && reinterpret_cast<uintptr_t>(out_nchw) % 16 == 0;
    const long long items = (long long)out_h * (vec ? out_w / 4 : out_w);
    const size_t plane = (size_t)out_h * out_w;
    for (int i0 = 0; i0 < n; i0 += OM_PRE_BATCH) {
        om::PreBatch bt;
        bt.n = n - i0 < OM_PRE_BATCH ? n - i0 : OM_PRE_BATCH;
        bt.out = out_nchw + (size_t)i0 * 3 * plane;
        bt.out_h = out_h; bt.out_w = out_w; bt.pad_value = pad_value;
        for (int c = 0; c < 3; ++c) { bt.mean[c] = mean3[c]; bt.stdv[c] = std3[c]; }
        for (int k = 0; k < OM_PRE_BATCH; ++k) {
            const int i = i0 + (k < bt.n ? k : 0);            // the unused entries repeat the first: no workgroup reads them
            const int32_t* g = geom + 8 * (size_t)i;
            om::PreImg& q = bt.img[k];
            q.src = images[i];
            q.h = g[0]; q.w = g[1]; q.rh = g[2]; q.rw = g[3]; q.pad_top = g[4]; q.pad_left = g[5]; q.flags = g[6];
            q.small_out = g[2] + g[3] <= om::BILINEAR_SMALL_OUT ? 1 : 0;
            q.scale_h = (float)g[0] / (float)g[2];            // area_pixel_compute_scale with size= given
            q.scale_w = (float)g[1] / (float)g[3];
        }
        const dim3 grid((unsigned)((items + 255) / 256), (unsigned)bt.n);
        if (vec)
            hipLaunchKernelGGL(om::preprocess_batch_kernel<4>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), bt);
        else
            hipLaunchKernelGGL(om::preprocess_batch_kernel<1>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), bt);
        OM_CHECK_HIP(hipGetLastError());
    }
    return OM_OK;
}

int om_pad_nchw(const float* in, long long planes, int h, int w, int pad_top, int pad_left, int out_h, int out_w,
                float pad_value, float* out, om_stream stream) {
    OM_REQUIRE(in && out && planes > 0 && h > 0 && w > 0, OM_EINVAL, "om_pad_nchw: bad argument");
    OM_REQUIRE(pad_top >= 0 && pad_left >= 0 && pad_top + h <= out_h && pad_left + w <= out_w, OM_EINVAL,
               "om_pad_nchw: the image does not fit the output");
    const long long total = planes * out_h * out_w;
    hipLaunchKernelGGL(om::pad_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), in, out, planes, h, w, out_h, out_w, pad_top, pad_left, pad_value);
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

}  // extern "C"
