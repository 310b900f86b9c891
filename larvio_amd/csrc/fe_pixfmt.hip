// fe_pixfmt.hip — lvk_image_to_gray: a camera's pixel format to the 8-bit grey plane the front-end reads (contract: include/lvk_c.h).
// Memory-bound and tiny: one launch, no LDS, no atomics.  Each lane produces one aligned dword of output from the 4 / 8 / 12 / 16 source
// bytes in front of it (consecutive lanes read consecutive runs: every fetched line is used whole), the per-lane arithmetic lives in
// fe_pixfmt_dev.h where a host harness runs it too.
#include "lvk_internal.h"
#include "fe_pixfmt_dev.h"

// grid: x over the lanes of a row (the widest row: 3 bytes of misalignment), y over rows, strided when h exceeds the grid
template <int FMT>
__global__ void __launch_bounds__(256) k_image_to_gray(const uint8_t* __restrict__ src, size_t sstride, int w, int h, int shift,
                                                       uint8_t* __restrict__ dst, size_t dstride)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    for (int y = blockIdx.y; y < h; y += gridDim.y)
        pixfmt_lane<FMT>(src + (size_t)y * sstride, dst + (size_t)y * dstride, w, shift, k);
}

lvk_status lvk_image_to_gray(lvk_context* ctx, const void* d_src, int src_stride_bytes, int w, int h, int format, int shift,
                             uint8_t* d_dst, int dst_stride)
{
    if (!ctx) return LVK_ERR_ARG;
    if (!d_src || !d_dst) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_image_to_gray: null pointer");
    if (w <= 0 || h <= 0) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_image_to_gray: %d x %d is not an image", w, h);
    const int bpp = lvk_pixfmt_bpp(format);
    if (!bpp) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_image_to_gray: unknown format %d", format);
    if ((long long)src_stride_bytes < (long long)w * bpp)
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_image_to_gray: source stride %d is smaller than a %s row of %d pixels (%lld bytes)", src_stride_bytes, lvk_pixfmt_name(format), w, (long long)w * bpp);
    if (dst_stride < w) return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_image_to_gray: destination stride %d is smaller than the width %d", dst_stride, w);
    if (shift < 0 || shift > 8 || (shift != 0 && format != LVK_PIX_MONO16))
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_image_to_gray: shift %d (0..8, and only with mono16; the format is %s)", shift, lvk_pixfmt_name(format));
    if ((format == LVK_PIX_YUYV || format == LVK_PIX_UYVY) && (w & 1))
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_image_to_gray: %s needs an even width, not %d", lvk_pixfmt_name(format), w);
    if (format == LVK_PIX_MONO16 && ((((uintptr_t)d_src) | (unsigned)src_stride_bytes) & 1u))
        return lvk_set_error(ctx, LVK_ERR_ARG, "lvk_image_to_gray: mono16 needs an even source address and stride");
    const dim3 grid((((unsigned)w + 3u + 3u) / 4u + 255u) / 256u,(unsigned)(h < 65535 ? h : 65535)), block(256);
    const uint8_t* s = (const uint8_t*)d_src;
    const size_t ss = (size_t)src_stride_bytes, ds = (size_t)dst_stride;
    switch (format) {
#define LVK_PIX_CASE(F) case F: hipLaunchKernelGGL(k_image_to_gray<F>, grid, block, 0, ctx->stream, s, ss, w, h, shift, d_dst, ds); break;
    LVK_PIX_CASE(LVK_PIX_MONO8) LVK_PIX_CASE(LVK_PIX_BGR8) LVK_PIX_CASE(LVK_PIX_RGB8) LVK_PIX_CASE(LVK_PIX_BGRA8)
    LVK_PIX_CASE(LVK_PIX_RGBA8) LVK_PIX_CASE(LVK_PIX_MONO16) LVK_PIX_CASE(LVK_PIX_YUYV) LVK_PIX_CASE(LVK_PIX_UYVY)
#undef LVK_PIX_CASE
    }
    LVK_LAUNCH_CHECK(ctx);
    return LVK_OK;
}
