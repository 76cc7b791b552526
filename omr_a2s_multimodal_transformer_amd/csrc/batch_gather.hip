// A padded batch from a device-resident training set (gfx950).  The set is ONE packed buffer: sample n is a row-major h_n x w_n plane
// of uint8 grays (a score image before its / 255) or of fp32 values (a spectrogram) that starts at element offsets[n]; sizes[n] =
// (h_n, w_n).  omr_gather_ragged_batch builds out[B][1][H][W] from a list of B sample indices in one launch:
//   out[b][0][i][j] = conv(src[offsets[n] + i * w_n + j]) for i < h_n, j < w_n, n = idx[b];  pad_value everywhere else
// -- the right/bottom padding of pad_batch_inputs (pad 1.0: the white background of the dense collate) and of image.collate_ragged
// (pad 0: what the ragged encoder expects outside an extent) with the / 255 of preprocess_image folded in.  conv(uint8 v) =
// __fdiv_rn((float)v, 255.0f), the expression of vpass_to_float_kernel (image.hip): the floats are image.preprocess_image's to the
// bit; an fp32 source is copied.  A bf16 plane holds from_f32<bf16> of those floats: omr_cast of the fp32 plane.
// Memory-bound, in the manner of pack_memory_kernel (extent.hip): blockIdx.y = b, the threads of a sample walk the destination plane
// linearly with a grid-stride loop, one 16-byte store per iteration where W is a multiple of the fragment width and out is 16-byte
// aligned (a fragment then never crosses a row), else one element.  Source rows start at any element offset (w_n is arbitrary), so
// the source is loaded element by element -- neighbouring lanes read neighbouring bytes.  Positions inside a sample are 32-bit
// (H * W <= 2^31 - 1, and h_n * w_n <= H * W after the clamp); only the batch offset and offsets[n] are 64-bit.  Of src exactly the
// h_n * w_n elements of each listed sample are read.  No LDS, no atomics.  (batch_augment.hip: the same launch with a per-sample
// augmentation; its identity record writes this kernel's bits.)
#include "omr_common.h"
#include "omr_hip.h"
#include "instnorm_slots.h"      // Pack, clampi
#include "batch_gather.h"        // gather_conv, gather_pad: shared with batch_augment.hip

namespace {

template <typename S, typename T, int VEC>
__global__ __launch_bounds__(256) void gather_ragged_batch_kernel(const S* __restrict__ src, const long* __restrict__ offsets, const int* __restrict__ sizes,
                                                                  int N, const int* __restrict__ idx, T* __restrict__ out, int H, int W, float pad_value) {
    typedef Pack<T, VEC> P;
    const int b = blockIdx.y;
    const int n = clampi(idx[b], 0, N - 1);
    const unsigned h = clampi(sizes[2 * n], 0, H), w = clampi(sizes[2 * n + 1], 0, W);
    const unsigned per = (unsigned)H * W / VEC;            // destination fragments of this sample
    const S* sb = src + offsets[n];
    T* ob = out + (long)b * H * W;
    const T pad = gather_pad<T>(pad_value);
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < per; t += gridDim.x * blockDim.x) {
        const unsigned pix = t * VEC, i = pix / (unsigned)W, j = pix - i * W;
        P o;
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = (i < h && j + e < w) ? from_f32<T>(gather_conv(sb[i * w + j + e])) : pad;
        *reinterpret_cast<P*>(ob + (long)t * VEC) = o;
    }
}

template <typename S, typename T, int VEC>
void launch_gather(const void* src, const long* offsets, const int* sizes, int N, const int* idx, void* out, int B, int H, int W, float pad_value,
                   hipStream_t s) {
    long gx = ((long)H * W / VEC + 255) / 256;          // per sample (blockIdx.y): at most 256 * 256 threads, the pack kernels' cap
    gx = gx < 1 ? 1 : (gx > 256 ? 256 : gx);
    hipLaunchKernelGGL((gather_ragged_batch_kernel<S, T, VEC>), dim3((unsigned)gx, B), 256, 0, s, (const S*)src, offsets, sizes, N, idx, (T*)out, H, W,
                       pad_value);
}

template <typename S>
int gather_dst(const void* src, const long* offsets, const int* sizes, int N, const int* idx, int dst_dtype, void* out, int B, int H, int W, float pad_value,
               hipStream_t s) {
    const bool aligned = (uintptr_t)out % 16 == 0;
    if (dst_dtype == OMR_F32) {
        if (aligned && W % 4 == 0) launch_gather<S, float, 4>(src, offsets, sizes, N, idx, out, B, H, W, pad_value, s);
        else launch_gather<S, float, 1>(src, offsets, sizes, N, idx, out, B, H, W, pad_value, s);
    } else if (dst_dtype == OMR_BF16) {
        if (aligned && W % 8 == 0) launch_gather<S, bf16, 8>(src, offsets, sizes, N, idx, out, B, H, W, pad_value, s);
        else launch_gather<S, bf16, 1>(src, offsets, sizes, N, idx, out, B, H, W, pad_value, s);
    } else return OMR_ERR_UNSUPPORTED;
    OMR_CHECK_LAUNCH();
    return OMR_OK;
}

}  // namespace

extern "C" int omr_gather_ragged_batch(int src_dtype, const void* src, const long* offsets, const int* sizes, int N, const int* idx, int dst_dtype,
                                       void* out, int B, int H, int W, float pad_value, void* stream) {
    if (!src || !offsets || !sizes || !idx || !out || N < 1 || B < 1 || B > 65535 || H < 1 || W < 1 || (long)H * W > 0x7fffffffL) return OMR_ERR_ARG;
    if (src_dtype == OMR_DTYPE_U8) return gather_dst<unsigned char>(src, offsets, sizes, N, idx, dst_dtype, out, B, H, W, pad_value, (hipStream_t)stream);
    if (src_dtype == OMR_F32) return gather_dst<float>(src, offsets, sizes, N, idx, dst_dtype, out, B, H, W, pad_value, (hipStream_t)stream);
    return OMR_ERR_UNSUPPORTED;
}
