// The single-layer entries of liborienmask_hip.so (include/orienmask_hip.h, "one convolution"): one launch each on caller-owned
// tensors, for the unit tests and the per-layer benchmarks.  Nothing here knows about a model.
#include "om_common.h"

namespace {

// What the entries own: each block is allocated once, on the device current at the first call that needs it, and never freed.
// Nothing locks or asks for the device again: callers are serialised and stay on that device.  Unit tests and benchmarks only;
// om_forward carves both from the caller's workspace.
int* g_ticket = nullptr;        // SYNC_WORDS ints, zeroed on the caller's stream before every launch: the persistent tile queue
float* g_partial = nullptr;     // om_conv2d_split_k: room for 512 parts of 128 x 64 floats

hipStream_t hs(om_stream s) { return static_cast<hipStream_t>(s); }

struct Layer {      // the arguments the entries share, in the ABI's order
    const void* in; int B, H, W, cin, in_pix_stride; const void* w; const float *scale, *shift; int cout, ks, stride, leaky;
    const void* res; int res_pix_stride; void* out; int out_pix_stride, out_mode = 0, up = 1;
};

// One entry's arguments become its ConvArgs / ConvArgsH: the shape requirement under the entry's name, then `more` (what else the
// entry requires before its launch), then pointers, the shape with cout rounded up to cout_to, and the zeroed ticket.  The entry
// sets what is its own after it, and launches.
template <class Args, class More>
int unit_args(Args& a, const char* who, const Layer& l, int cout_to, om_stream stream, More more) {
    OM_REQUIRE(l.B > 0 && l.H > 0 && l.W > 0 && l.stride >= 1 && l.H % l.stride == 0 && l.W % l.stride == 0, OM_EINVAL, "%s: bad shape", who);
    if (int rc = more()) return rc;
    a.in = static_cast<decltype(a.in)>(l.in); a.w = static_cast<decltype(a.w)>(l.w); a.scale = l.scale; a.shift = l.shift;
    a.res = static_cast<decltype(a.res)>(l.res); a.out = static_cast<decltype(a.out)>(l.out);
    om::fill_conv_shape(a, l.B, l.H, l.W, l.cin, l.in_pix_stride, l.cout, om::round_up(l.cout, cout_to), l.ks, l.stride, l.leaky, l.res_pix_stride, l.out_pix_stride, l.out_mode, l.up);
    if (!g_ticket) OM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&g_ticket), om::SYNC_WORDS * sizeof(int)));
    a.ticket = g_ticket;
    return om::launch_zero_words(g_ticket, om::SYNC_WORDS, hs(stream));
}

int require_out_mode(const char* who, const Layer& l) {
    OM_REQUIRE(l.out_mode >= 0 && l.out_mode <= 2 && l.up >= 1 && (l.out_mode == 1 || l.up == 1), OM_EINVAL,
               "%s: out_mode=%d up=%d (0 NHWC, 1 NHWC replicated up x up, 2 NCHW)", who, l.out_mode, l.up);
    return OM_OK;
}

int require_scratch(const char* who, const void* scratch, size_t have, size_t need) {
    OM_REQUIRE(scratch && have >= need, OM_ENOMEM, "%s: scratch too small", who);
    return OM_OK;
}

// om_conv2d_split, and om_conv2d_split_k (by_k): a tile's k loop in up to max_parts parts, partial sums in g_partial
int conv2d_split_impl(const char* who, const Layer& l, int tile_bm, int tile_bn, bool by_k, int max_parts, int32_t* status_dev, om_stream stream) {
    om::ConvArgs a;
    if (int rc = unit_args(a, who, l, 32, stream, [&]() -> int {
            if (int rc = require_out_mode(who, l)) return rc;
            OM_REQUIRE(!by_k || (max_parts >= 1 && max_parts <= 8), OM_EINVAL, "%s: max_parts=%d (1 .. 8)", who, max_parts);
            if (by_k && !g_partial) OM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&g_partial), (size_t)512 * 128 * 64 * sizeof(float)));
            return OM_OK;
        })) return rc;
    a.force_bm = tile_bm; a.force_bn = tile_bn; a.status = status_dev;
    if (by_k) { a.ksplit_max = max_parts; a.sk_partial = g_partial; }
    return om::launch_conv_igemm_split(a, hs(stream));
}

// om_conv2d_winograd24 and its split-operand form; both report under the first one's name
int conv2d_winograd24_impl(const Layer& l, void* scratch, size_t scratch_bytes, int split, int32_t* status_dev, om_stream stream) {
    om::ConvArgs a;
    if (int rc = unit_args(a, "om_conv2d_winograd24", l, 64, stream, [&] {
            return require_scratch("om_conv2d_winograd24", scratch, scratch_bytes, om_conv2d_winograd24_scratch_bytes(l.B, l.H, l.W, l.cin));
        })) return rc;
    a.split = split; a.status = status_dev;
    a.sk_partial = reinterpret_cast<float*>(static_cast<char*>(scratch) + om::align_up(om::wino24_scratch_floats(l.B, l.H, l.W, l.cin) * sizeof(float), 256));
    return om::launch_conv_winograd24(a, static_cast<float*>(scratch), hs(stream));
}

// om_conv2d_wino14_split: the fused kernel, no scratch; om_conv2d_wino14_wide: the V pre-pass into `scratch`, then the wide kernel
int conv2d_wino14_impl(const char* who, const Layer& l, bool wide, void* scratch, size_t scratch_bytes, int32_t* status_dev, om_stream stream) {
    om::ConvArgs a;
    if (int rc = unit_args(a, who, l, 64, stream, [&] {
            return wide ? require_scratch(who, scratch, scratch_bytes, om_conv2d_wino14_wide_scratch_bytes(l.B, l.H, l.W, l.cin)) : OM_OK;
        })) return rc;
    a.split = 1; a.status = status_dev;
    return wide ? om::launch_conv_wino14_wide(a, static_cast<float*>(scratch), hs(stream)) : om::launch_conv_wino14_split(a, hs(stream));
}

}  // namespace

extern "C" {

int om_conv2d_mode(const float* in, int B, int H, int W, int cin, int in_pix_stride, const float* w, const float* scale,
                   const float* shift, int cout, int ksize, int stride, int leaky, const float* res, int res_pix_stride, float* out,
                   int out_pix_stride, int out_mode, int up, om_stream stream) {
    const Layer l{in, B, H, W, cin, in_pix_stride, w, scale, shift, cout, ksize, stride, leaky, res, res_pix_stride, out, out_pix_stride, out_mode, up};
    om::ConvArgs a;
    if (int rc = unit_args(a, "om_conv2d", l, 32, stream, [&] { return require_out_mode("om_conv2d_mode", l); })) return rc;
    return om::launch_conv_igemm(a, hs(stream));
}

int om_conv2d(const float* in, int B, int H, int W, int cin, int in_pix_stride, const float* w, const float* scale, const float* shift,
              int cout, int ksize, int stride, int leaky, const float* res, int res_pix_stride, float* out, int out_pix_stride,
              om_stream stream) {
    return om_conv2d_mode(in, B, H, W, cin, in_pix_stride, w, scale, shift, cout, ksize, stride, leaky, res, res_pix_stride, out,
                          out_pix_stride, 0, 1, stream);
}

int om_conv2d_split(const float* in, int B, int H, int W, int cin, int in_pix_stride, const void* w_split, const float* scale_split,
                    const float* shift, int cout, int ksize, int stride, int leaky, const float* res, int res_pix_stride, float* out,
                    int out_pix_stride, int out_mode, int up, int tile_bm, int tile_bn, int32_t* status_dev, om_stream stream) {
    const Layer l{in, B, H, W, cin, in_pix_stride, w_split, scale_split, shift, cout, ksize, stride, leaky, res, res_pix_stride, out, out_pix_stride, out_mode, up};
    return conv2d_split_impl("om_conv2d_split", l, tile_bm, tile_bn, false, 0, status_dev, stream);
}

int om_conv2d_split_k(const float* in, int B, int H, int W, int cin, int in_pix_stride, const void* w_split, const float* scale_split,
                      const float* shift, int cout, int ksize, int stride, int leaky, const float* res, int res_pix_stride, float* out,
                      int out_pix_stride, int out_mode, int up, int tile_bm, int tile_bn, int max_parts, int32_t* status_dev,
                      om_stream stream) {
    const Layer l{in, B, H, W, cin, in_pix_stride, w_split, scale_split, shift, cout, ksize, stride, leaky, res, res_pix_stride, out, out_pix_stride, out_mode, up};
    return conv2d_split_impl("om_conv2d_split_k", l, tile_bm, tile_bn, true, max_parts, status_dev, stream);
}

// The input is a segment table, not one view: requirements of its own around the shared steps
int om_conv2d_split_gather(int nseg, const float* const* seg_ptr, const int* seg_channels, const int* seg_pix_stride, const int* seg_up,
                           int B, int H, int W, const void* w_split, const float* scale_split, const float* shift, int cout, int leaky,
                           float* out, int out_pix_stride, int32_t* status_dev, om_stream stream) {
    OM_REQUIRE(B > 0 && H > 0 && W > 0 && nseg >= 1 && nseg <= 4 && seg_ptr && seg_channels && seg_pix_stride && seg_up, OM_EINVAL,
               "om_conv2d_split_gather: bad shape / null segment table (nseg=%d)", nseg);
    om::ConvArgs a;
    a.nseg = nseg;
    int cin = 0;
    for (int g = 0; g < nseg; ++g) {
        a.seg_ptr[g] = seg_ptr[g]; a.seg_channels[g] = seg_channels[g]; a.seg_pix_stride[g] = seg_pix_stride[g]; a.seg_up[g] = seg_up[g];
        cin += seg_channels[g];
    }
    const Layer l{nullptr, B, H, W, cin, 0, w_split, scale_split, shift, cout, 1, 1, leaky, nullptr, 0, out, out_pix_stride};
    if (int rc = unit_args(a, "om_conv2d_split_gather", l, 32, stream, [&]() -> int {
            OM_REQUIRE(cin > 0 && cin % 32 == 0, OM_EINVAL, "om_conv2d_split_gather: %d input channels", cin);
            return OM_OK;
        })) return rc;
    a.status = status_dev;
    return om::launch_conv_igemm_split(a, hs(stream));
}

size_t om_conv2d_winograd_scratch_bytes(int B, int H, int W, int cin) {
    if (B <= 0 || H <= 0 || W <= 0 || cin <= 0) return 0;
    return om::align_up(om::wino_scratch_floats(B, H, W, cin) * sizeof(float), 256);
}
int om_conv2d_winograd(const float* in, int B, int H, int W, int cin, int in_pix_stride, const float* u, const float* scale,
                       const float* shift, int cout, int leaky, const float* res, int res_pix_stride, float* out, int out_pix_stride,
                       void* scratch, size_t scratch_bytes, om_stream stream) {
    const Layer l{in, B, H, W, cin, in_pix_stride, u, scale, shift, cout, 3, 1, leaky, res, res_pix_stride, out, out_pix_stride};
    om::ConvArgs a;
    if (int rc = unit_args(a, "om_conv2d_winograd", l, 64, stream, [&] {
            return require_scratch("om_conv2d_winograd", scratch, scratch_bytes, om_conv2d_winograd_scratch_bytes(B, H, W, cin));
        })) return rc;
    return om::launch_conv_winograd(a, static_cast<float*>(scratch), hs(stream));
}

int om_conv2d_f16(const void* in, int B, int H, int W, int cin, int in_pix_stride, const void* w, const float* scale,
                  const float* shift, int cout, int ksize, int stride, int leaky, const void* res, int res_pix_stride, void* out,
                  int out_pix_stride, int out_f32, om_stream stream) {
    const Layer l{in, B, H, W, cin, in_pix_stride, w, scale, shift, cout, ksize, stride, leaky, res, res_pix_stride, out, out_pix_stride};
    om::ConvArgsH a;
    if (int rc = unit_args(a, "om_conv2d_f16", l, 32, stream, [] { return 0; })) return rc;
    a.out_f32 = out_f32;
    return om::launch_conv_igemm_f16(a, hs(stream));
}

size_t om_conv2d_winograd24_scratch_bytes(int B, int H, int W, int cin) {
    if (B <= 0 || H <= 0 || W <= 0 || cin <= 0) return 0;
    return om::align_up(om::wino24_scratch_floats(B, H, W, cin) * sizeof(float), 256) + om::SK_PARTIAL_BYTES;
}
int om_conv2d_winograd24(const float* in, int B, int H, int W, int cin, int in_pix_stride, const float* u, const float* scale,
                         const float* shift, int cout, int leaky, const float* res, int res_pix_stride, float* out, int out_pix_stride,
                         void* scratch, size_t scratch_bytes, om_stream stream) {
    const Layer l{in, B, H, W, cin, in_pix_stride, u, scale, shift, cout, 3, 1, leaky, res, res_pix_stride, out, out_pix_stride};
    return conv2d_winograd24_impl(l, scratch, scratch_bytes, 0, nullptr, stream);
}

int om_conv2d_winograd24_split(const float* in, int B, int H, int W, int cin, int in_pix_stride, const void* u_split,
                               const float* scale_split, const float* shift, int cout, int leaky, const float* res, int res_pix_stride,
                               float* out, int out_pix_stride, void* scratch, size_t scratch_bytes, int32_t* status_dev,
                               om_stream stream) {
    const Layer l{in, B, H, W, cin, in_pix_stride, u_split, scale_split, shift, cout, 3, 1, leaky, res, res_pix_stride, out, out_pix_stride};
    return conv2d_winograd24_impl(l, scratch, scratch_bytes, 1, status_dev, stream);
}

int om_conv2d_wino14_split(const float* in, int B, int H, int W, int cin, int in_pix_stride, const void* u14_split,
                           const float* scale_split, const float* shift, int cout, int leaky, const float* res, int res_pix_stride,
                           float* out, int out_pix_stride, int32_t* status_dev, om_stream stream) {
    const Layer l{in, B, H, W, cin, in_pix_stride, u14_split, scale_split, shift, cout, 3, 1, leaky, res, res_pix_stride, out, out_pix_stride};
    return conv2d_wino14_impl("om_conv2d_wino14_split", l, false, nullptr, 0, status_dev, stream);
}

int om_conv2d_wino14_blocks(int B, int H, int W, int* classes, int* row_pitch, long long* m_tiles) {
    OM_REQUIRE(B > 0 && H > 0 && W > 0 && classes && row_pitch && m_tiles, OM_EINVAL, "om_conv2d_wino14_blocks: bad argument");
    om::Wino14Class cls[om::W14_MAXCLS];
    long long gtot = 0;
    const int n = om::wino14_blocks(B, H, W, cls, row_pitch, &gtot, m_tiles);
    for (int k = 0; k < n; ++k) {
        const int v[5] = {cls[k].t0, cls[k].Ct, cls[k].ncb, cls[k].R, cls[k].nrb};
        for (int i = 0; i < 5; ++i) classes[5 * k + i] = v[i];
    }
    return n;
}

size_t om_conv2d_wino14_wide_scratch_bytes(int B, int H, int W, int cin) {
    if (B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cin % 16) return 0;
    return om::align_up(om::wino14_wide_scratch_floats(B, H, W, cin) * sizeof(float), 256);
}
int om_conv2d_wino14_wide(const float* in, int B, int H, int W, int cin, int in_pix_stride, const void* u14_split,
                          const float* scale_split, const float* shift, int cout, int leaky, const float* res, int res_pix_stride,
                          float* out, int out_pix_stride, void* scratch, size_t scratch_bytes, int32_t* status_dev, om_stream stream) {
    const Layer l{in, B, H, W, cin, in_pix_stride, u14_split, scale_split, shift, cout, 3, 1, leaky, res, res_pix_stride, out, out_pix_stride};
    return conv2d_wino14_impl("om_conv2d_wino14_wide", l, true, scratch, scratch_bytes, status_dev, stream);
}

int om_conv2d_stem(const float* in, int B, int H, int W, const float* w, const float* scale, const float* shift, int cout, float* out,
                   om_stream stream) {
    return om::launch_conv_stem(in, B, H, W, w, scale, shift, cout, out, hs(stream));
}

int om_conv2d_stem_f16(const float* in, int B, int H, int W, const float* w, const float* scale, const float* shift, int cout,
                       void* out, om_stream stream) {
    return om::launch_conv_stem_f16(in, B, H, W, w, scale, shift, cout, out, hs(stream));
}

int om_conv2d_stem2_split(const float* in, int B, int H, int W, const float* w1, const float* scale1, const float* shift1,
                          const void* w2_split, const float* scale2_split, const float* shift2, int cout2, int leaky2, float* out,
                          int out_pix_stride, int32_t* status_dev, om_stream stream) {
    return om::launch_conv_stem2_split(in, B, H, W, w1, scale1, shift1, w2_split, scale2_split, shift2, cout2, leaky2, out,
                                       out_pix_stride, status_dev, hs(stream));
}

int om_conv2d_stem3_split(const float* in, int B, int H, int W, const float* w1, const float* scale1, const float* shift1,
                          const void* w2_split, const float* scale2_split, const float* shift2, int cout2, int leaky2, float* out,
                          int out_pix_stride, const void* w3_split, const float* scale3_split, const float* shift3, int cout3,
                          int leaky3, float* out3, int out3_pix_stride, int32_t* status_dev, om_stream stream) {
    om::Stem2Third third{w3_split, scale3_split, shift3, out3, cout3, leaky3, out3_pix_stride};
    return om::launch_conv_stem2_split(in, B, H, W, w1, scale1, shift1, w2_split, scale2_split, shift2, cout2, leaky2, out,
                                       out_pix_stride, status_dev, hs(stream), &third);
}

int om_conv2d_stem2_f16(const float* in, int B, int H, int W, const float* w1, const float* scale1, const float* shift1,
                        const void* w2_f16, const float* scale2, const float* shift2, int cout2, int leaky2, void* out,
                        int out_pix_stride, om_stream stream) {
    return om::launch_conv_stem2_f16(in, B, H, W, w1, scale1, shift1, w2_f16, scale2, shift2, cout2, leaky2, out, out_pix_stride, hs(stream));
}

}  // extern "C"
