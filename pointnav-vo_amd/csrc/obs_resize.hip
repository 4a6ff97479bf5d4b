// obs_resize.hip — observation resize + center crop on the device (VO.OBS_TRANSFORM / RL.OBS_TRANSFORM), gfx950 only.
//
// The reference transforms sensor frames with F.interpolate(mode="area") (pointnav_vo/utils/misc_utils.py:241-288,
// image_resize_shortest_edge) followed by a slice (center_crop, :291-318).  Area interpolation is adaptive_avg_pool2d:
//   output (oy, ox) averages input rows [floor(oy*Hi/Ho), ceil((oy+1)*Hi/Ho)) and columns likewise,
//   summed in float32 in order (input row outer, input column inner, one rounding per add),
// then divided by the window size with one of torch's two CPU rules, chosen by the memory format torch receives:
//   div_rule 0 (contiguous NCHW kernel):      (sum / kh) / kw
//   div_rule 1 (channels-last NHWC kernel):   sum / (kh * kw)
// This file is built with -ffp-contract=off (no a*b+c fusion) and without fast-math, so '/' is the correctly rounded IEEE
// division (v_div_scale / v_div_fmas / v_div_fixup), never a reciprocal multiply: the results are bit-exact to torch's.
//
// One launch covers N frames.  The crop is an offset into the resized grid: only the output pixels inside the crop window are
// computed, and the resized grid is never materialised.  A workgroup owns (frame, band of R output rows): it stages the
// input rows the band's windows touch — only the columns the crop window touches — into LDS once, with 16-byte loads where the
// row is packed, then computes every output of the band from LDS.  Adjacent output rows share input rows at non-integer ratios,
// so each input byte is read from HBM once (plus at most one shared row per band boundary).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/pnvo.h"
#include "pnvo_internal.h"
#include "pnvo_model.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxC = 4;
constexpr size_t kLdsBudget = 48 * 1024;     // bytes of LDS per workgroup (3 workgroups per CU)

__host__ __device__ inline int win_lo(int o, int out_n, int in_n) { return (int)(((int64_t)o * in_n) / out_n); }
__host__ __device__ inline int win_hi(int o, int out_n, int in_n) {
  return (int)((((int64_t)(o + 1) * in_n) + out_n - 1) / out_n);
}

struct ResizeArgs {
  const uint8_t *src;
  int esize;                 // 1: uint8, 4: float32
  int in_h, in_w, C;
  int64_t s_frame, s_row, s_pix;        // element strides of the source
  int rs_h, rs_w;                       // resized grid
  int crop_y, crop_x, out_h, out_w;     // crop window inside the resized grid
  float *dst;
  int group;                            // frames per destination group (2: pairs)
  int64_t d_group, d_member, d_row, d_pix;   // element strides of the destination
  int rows_per_band;
  int col_lo, col_hi;                   // input columns the crop window touches
  int lds_pitch;                        // bytes per staged row
  int packed;                           // s_pix == C: a row segment is contiguous bytes
  int div_rule;
};

template <typename T>
__device__ inline float ld_lds(const uint8_t *p) {
  return (float)(*reinterpret_cast<const T *>(p));
}

template <typename T>
__global__ void __launch_bounds__(kThreads) resize_area_kernel(ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int f = blockIdx.y;
  const int oy0 = blockIdx.x * a.rows_per_band;
  const int oy1 = min(oy0 + a.rows_per_band, a.out_h);
  const int ih_lo = win_lo(oy0 + a.crop_y, a.rs_h, a.in_h);
  const int ih_hi = win_hi(oy1 - 1 + a.crop_y, a.rs_h, a.in_h);
  const int nrows = ih_hi - ih_lo;
  const int ncols = a.col_hi - a.col_lo;
  const int seg = ncols * a.C * a.esize;                      // bytes of one staged row
  const uint8_t *src_f = a.src + (size_t)f * a.s_frame * a.esize;
  // byte offset of staged row r inside its LDS row: the segment's own 16-byte misalignment (packed rows), else 0
  auto lead_of = [&](int r) -> int {
    return a.packed ? (int)((uintptr_t)(src_f + ((size_t)(ih_lo + r) * a.s_row + (size_t)a.col_lo * a.s_pix) * a.esize) & 15) : 0;
  };

  // ---- stage the band's input rows (crop columns only) into LDS
  if (a.packed) {
    for (int r = 0; r < nrows; ++r) {
      const uint8_t *g = src_f + ((size_t)(ih_lo + r) * a.s_row + (size_t)a.col_lo * a.s_pix) * a.esize;
      const int lead = lead_of(r);
      const int head = min((16 - lead) & 15, seg);
      const int body = (seg - head) >> 4;
      const int tail = seg - head - (body << 4);
      uint8_t *l = lds + (size_t)r * a.lds_pitch + lead;    // LDS row base is 16-aligned: l and g share their alignment
      for (int t = threadIdx.x; t < head + body + tail; t += kThreads) {
        if (t < head) {
          l[t] = g[t];
        } else if (t < head + body) {
          const int b = head + ((t - head) << 4);
          *reinterpret_cast<uint4 *>(l + b) = *reinterpret_cast<const uint4 *>(g + b);
        } else {
          const int b = head + (body << 4) + (t - head - body);
          l[b] = g[b];
        }
      }
    }
  } else {
    const int per_row = ncols * a.C;
    for (int t = threadIdx.x; t < nrows * per_row; t += kThreads) {
      const int r = t / per_row, e = t - r * per_row;
      const int col = e / a.C, c = e - col * a.C;
      const T *g = reinterpret_cast<const T *>(src_f) + (size_t)(ih_lo + r) * a.s_row + (size_t)(a.col_lo + col) * a.s_pix + c;
      *reinterpret_cast<T *>(lds + (size_t)r * a.lds_pitch + (size_t)e * sizeof(T)) = *g;
    }
  }
  __syncthreads();

  // ---- one output pixel (all channels) per thread and iteration
  float *dst_f = a.dst + (size_t)(f / a.group) * a.d_group + (size_t)(f % a.group) * a.d_member;
  const int nout = (oy1 - oy0) * a.out_w;
  for (int t = threadIdx.x; t < nout; t += kThreads) {
    const int oy = oy0 + t / a.out_w, ox = t % a.out_w;
    const int y0 = win_lo(oy + a.crop_y, a.rs_h, a.in_h), y1 = win_hi(oy + a.crop_y, a.rs_h, a.in_h);
    const int x0 = win_lo(ox + a.crop_x, a.rs_w, a.in_w), x1 = win_hi(ox + a.crop_x, a.rs_w, a.in_w);
    float sum[kMaxC] = {0.f, 0.f, 0.f, 0.f};
    for (int y = y0; y < y1; ++y) {
      const uint8_t *row = lds + (size_t)(y - ih_lo) * a.lds_pitch + lead_of(y - ih_lo);
      for (int x = x0; x < x1; ++x) {
        const uint8_t *px = row + (size_t)(x - a.col_lo) * a.C * sizeof(T);
#pragma unroll
        for (int c = 0; c < kMaxC; ++c)
          if (c < a.C) sum[c] = sum[c] + ld_lds<T>(px + c * sizeof(T));
      }
    }
    const int kh = y1 - y0, kw = x1 - x0;
    float *o = dst_f + (size_t)oy * a.d_row + (size_t)ox * a.d_pix;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) {
      if (c < a.C) o[c] = a.div_rule ? sum[c] / (float)(kh * kw) : (sum[c] / (float)kh) / (float)kw;
    }
  }
}

}  // namespace

extern "C" int pnvo_resize_area(const void *src, int src_dtype, int n, int in_h, int in_w, int channels, int64_t src_frame_stride,
                                int64_t src_row_stride, int64_t src_pix_stride, int rs_h, int rs_w, int crop_y, int crop_x, int out_h,
                                int out_w, float *dst, int dst_group, int64_t dst_group_stride, int64_t dst_member_stride,
                                int64_t dst_row_stride, int64_t dst_pix_stride, int div_rule, void *stream) {
  if (!src || !dst || n < 0 || in_h <= 0 || in_w <= 0 || channels < 1 || channels > kMaxC || rs_h <= 0 || rs_w <= 0 || out_h <= 0 ||
      out_w <= 0 || dst_group < 1 || (src_dtype != 0 && src_dtype != 1) || (div_rule != 0 && div_rule != 1))
    return pnvo_fail(nullptr, PNVO_ERR_ARG, "pnvo_resize_area: bad argument");
  if (crop_y < 0 || crop_x < 0 || crop_y + out_h > rs_h || crop_x + out_w > rs_w)
    return pnvo_fail(nullptr, PNVO_ERR_ARG, "pnvo_resize_area: crop window " + std::to_string(out_h) + "x" + std::to_string(out_w) + " at (" +
                                           std::to_string(crop_y) + "," + std::to_string(crop_x) + ") outside the resized " +
                                           std::to_string(rs_h) + "x" + std::to_string(rs_w) + " grid");
  if (src_pix_stride < channels || src_row_stride < (int64_t)in_w * src_pix_stride ||
      (n > 1 && src_frame_stride < (int64_t)in_h * src_row_stride))
    return pnvo_fail(nullptr, PNVO_ERR_ARG, "pnvo_resize_area: source strides overlap");
  if (dst_pix_stride < channels || dst_row_stride < (int64_t)out_w * dst_pix_stride)
    return pnvo_fail(nullptr, PNVO_ERR_ARG, "pnvo_resize_area: destination strides overlap");
  if (n == 0) return PNVO_OK;

  ResizeArgs a;
  a.src = static_cast<const uint8_t *>(src);
  a.esize = src_dtype == 0 ? 1 : 4;
  a.in_h = in_h, a.in_w = in_w, a.C = channels;
  a.s_frame = src_frame_stride, a.s_row = src_row_stride, a.s_pix = src_pix_stride;
  a.rs_h = rs_h, a.rs_w = rs_w, a.crop_y = crop_y, a.crop_x = crop_x, a.out_h = out_h, a.out_w = out_w;
  a.dst = dst;
  a.group = dst_group, a.d_group = dst_group_stride, a.d_member = dst_member_stride, a.d_row = dst_row_stride, a.d_pix = dst_pix_stride;
  a.col_lo = win_lo(crop_x, rs_w, in_w);
  a.col_hi = win_hi(crop_x + out_w - 1, rs_w, in_w);
  a.packed = src_pix_stride == channels;
  a.div_rule = div_rule;
  const int seg = (a.col_hi - a.col_lo) * channels * a.esize;
  a.lds_pitch = ((seg + 15) / 16 + 1) * 16;                   // + 16: room for the segment's misalignment
  // the largest band (output rows per workgroup) whose staged input rows fit the LDS budget
  size_t lds = 0;
  int R = 16;
  for (; R >= 1; R /= 2) {
    int most = 0;
    for (int oy0 = 0; oy0 < out_h; oy0 += R) {
      const int oy1 = oy0 + R < out_h ? oy0 + R : out_h;
      const int rows = win_hi(oy1 - 1 + crop_y, rs_h, in_h) - win_lo(oy0 + crop_y, rs_h, in_h);
      most = rows > most ? rows : most;
    }
    lds = (size_t)most * a.lds_pitch;
    if (lds <= kLdsBudget) break;
  }
  if (R < 1)
    return pnvo_fail(nullptr, PNVO_ERR_ARG, "pnvo_resize_area: one output row needs " + std::to_string(lds) +
                                           " bytes of staged input, over the 48 KiB LDS budget");
  a.rows_per_band = R;
  const dim3 grid((unsigned)((out_h + R - 1) / R), (unsigned)n);
  if (src_dtype == 0)
    hipLaunchKernelGGL(resize_area_kernel<uint8_t>, grid, dim3(kThreads), lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(resize_area_kernel<float>, grid, dim3(kThreads), lds, (hipStream_t)stream, a);
  HIPCHK(nullptr, hipGetLastError());
  return PNVO_OK;
}
