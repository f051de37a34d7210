// Ground-truth segmentations decoded on the device (orienmask_amd/augment.py: samples that carry 'segm'): what the reference's
// data/dataset.py does per annotation with pycocotools' frPyObjects / merge / decode, written as the row-packed bits that
// aug_mask_kernel (augment.hip) reads -- np.packbits(mask > 0, axis=1).
//
// Stage 1 is cocoeval.hip's (launch_coco_raster): every source -- a polygon, uncompressed counts, a compressed string -- becomes a
// column-major bitmap of its own: with hw = ceil(h/32), word x * hw + yb holds rows 32 yb .. 32 yb + 31 of column x, bit r = row
// 32 yb + r, the bits past row h zero.
//
//   segm_pack_kernel    stage 2.  One wave per tile of 32 rows x 64 columns of one mask: lane x loads word (x0 + x, yb) of each of
//                       the mask's sources and ORs them (maskUtils.merge: no merged bitmap is ever written); the ballot of bit r
//                       over the wave is row r's 64 columns; two lanes per row turn it into that row's 8 bytes, MSB first, and
//                       store them.  Lanes past column w hold zero, so the pad bits of a row's last byte are zero; a tile stores
//                       min(8, ceil(w/8) - x0/8) bytes of each of its rows below h, so every byte of the mask is written exactly
//                       once and none outside it.  No atomics, no LDS.
//
// Built with -ffp-contract=off like cocoeval.hip (the polygon arithmetic lives there; nothing here is floating point).
#include "om_common.h"

namespace om {

constexpr int SEGM_PACK_THREADS = 256;          // four waves
constexpr int SEGM_PACK_BLOCKS = 8;             // workgroups per mask; their waves stride over the mask's tiles

__global__ __launch_bounds__(SEGM_PACK_THREADS) void segm_pack_kernel(const int32_t* mask_hw, const int32_t* mask_src_first,
                                                                      const int64_t* mask_src_word_off, const int64_t* mask_out_off,
                                                                      const uint32_t* bitmaps, uint8_t* out) {
    const int m = blockIdx.y, lane = threadIdx.x & 63;
    const int h = mask_hw[2 * m], w = mask_hw[2 * m + 1], hw = (h + 31) >> 5, wb = (w + 7) >> 3;
    const int s0 = mask_src_first[m], s1 = mask_src_first[m + 1];
    const int n_tiles = hw * ((w + 63) >> 6);
    uint8_t* dst = out + mask_out_off[m];
    const int row_of_lane = lane >> 1, half = lane & 1;        // lanes 2r and 2r + 1 store row r's bytes 0..3 and 4..7
    // tile t = (column group t / hw, row band t % hw): neighbouring waves read neighbouring words of the same columns
    for (int t = blockIdx.x * (SEGM_PACK_THREADS / 64) + (threadIdx.x >> 6); t < n_tiles; t += gridDim.x * (SEGM_PACK_THREADS / 64)) {
        const int yb = t % hw, x0 = (t / hw) << 6, x = x0 + lane;
        uint32_t v = 0;
        if (x < w) {
            for (int s = s0; s < s1; ++s) v |= bitmaps[mask_src_word_off[s] + (long long)x * hw + yb];
        }
        uint32_t mine = 0;                                      // this lane's half of its row's 64 columns: bit i = column 32 half + i
        for (int r = 0; r < 32; ++r) {
            const unsigned long long cols = __ballot((v >> r) & 1u);
            const uint32_t part = half ? (uint32_t)(cols >> 32) : (uint32_t)cols;
            if (row_of_lane == r) mine = part;
        }
        // column 8 j + k of the half belongs in bit 7 - k of byte j: the bits of each byte reversed, the bytes in place
        const uint32_t packed = __builtin_bswap32(__brev(mine));
        const int y = 32 * yb + row_of_lane;
        const int n_bytes = min(8, wb - (x0 >> 3)) - 4 * half;  // of this lane's four
        if (y < h && n_bytes > 0) {
            uint8_t* p = dst + (long long)y * wb + (x0 >> 3) + 4 * half;
            if (n_bytes >= 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
                *reinterpret_cast<uint32_t*>(p) = packed;       // ceil(w/8) and the mask's offset have no alignment: only where it holds
            } else {
                for (int j = 0; j < min(n_bytes, 4); ++j) p[j] = (uint8_t)(packed >> 8 * j);
            }
        }
    }
}

}  // namespace om


extern "C" {

size_t om_segm_decode_workspace_bytes(long long bitmap_words, int n_masks) {
    if (bitmap_words < 0 || n_masks < 0) return 0;
    return om::align_up((size_t)bitmap_words * 4, 256);
}

int om_segm_decode(int n_masks, const int32_t* mask_hw, const int32_t* mask_src_first, const int64_t* mask_src_word_off,
                   const int64_t* mask_out_off, int n_poly, int n_srcs, const int32_t* src_kind, const int32_t* src_mask,
                   const int64_t* src_data_off, const int32_t* src_len, const int64_t* src_word_off, const double* poly,
                   const uint32_t* counts, const uint8_t* strings, long long bitmap_words, void* workspace, size_t ws_bytes,
                   uint8_t* out, om_stream stream) {
    OM_REQUIRE(n_masks >= 0 && n_masks <= 65535, OM_EINVAL, "om_segm_decode: n_masks = %d outside 0...65535", n_masks);
    OM_REQUIRE(n_poly >= 0 && n_srcs >= n_poly && bitmap_words >= 0, OM_EINVAL, "om_segm_decode: bad argument");
    if (n_masks == 0) return OM_OK;
    OM_REQUIRE(mask_hw && mask_src_first && mask_out_off && out && (n_srcs == 0 || mask_src_word_off), OM_EINVAL,
               "om_segm_decode: null pointer");
    OM_REQUIRE(n_srcs == 0 || (src_kind && src_mask && src_data_off && src_len && src_word_off), OM_EINVAL,
               "om_segm_decode: null source pointer");
    OM_REQUIRE(n_srcs == n_poly || counts || strings, OM_EINVAL, "om_segm_decode: sequences without data");
    OM_REQUIRE(bitmap_words == 0 || workspace, OM_EINVAL, "om_segm_decode: null workspace");
    const size_t need = om_segm_decode_workspace_bytes(bitmap_words, n_masks);
    OM_REQUIRE(ws_bytes >= need, OM_ENOMEM, "om_segm_decode: workspace of %zu bytes, %zu needed", ws_bytes, need);
    OM_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 4 == 0, OM_EINVAL, "om_segm_decode: workspace not 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t* bitmaps = static_cast<uint32_t*>(workspace);
    if (n_srcs > 0 && bitmap_words > 0) {
        const int rc = om::launch_coco_raster("om_segm_decode", n_poly, n_srcs, src_kind, src_mask, src_data_off, src_len, src_word_off,
                                              mask_hw, poly, counts, strings, bitmaps, bitmap_words, st);
        if (rc != OM_OK) return rc;
    }
    hipLaunchKernelGGL(om::segm_pack_kernel, dim3(om::SEGM_PACK_BLOCKS, n_masks), dim3(om::SEGM_PACK_THREADS), 0, st, mask_hw,
                       mask_src_first, mask_src_word_off, mask_out_off, bitmaps, out);
    OM_CHECK_HIP(hipGetLastError());
    return OM_OK;
}

}  // extern "C"
