// Resize of a resident batch to the model's image size, fused with the crop box and the flip of the pretraining
// augmentation: (B, C, Si, Si) -> (B, C, So, So).  The reference does this on the host with RandomResizedCrop(size) for
// training and Resize(size) + CenterCrop(size) for evaluation (src/data.py:15-34); here it sits between the uint8 dataset
// and the engine's pixel readers.  Per image a box (top, left, h, w) in source pixels and a flip flag (params NULL: the whole
// image, not flipped); per axis (x shown, ox' = So - 1 - ox under a flip), with s = w / So:
//   c = left + w (2 ox' + 1) / (2 So) - 0.5                       the source coordinate of the output pixel's centre
//   w <= So: c clamped to [0, Si - 1]; taps floor(c) and min(floor(c) + 1, Si - 1) with weights (1 - a, a), a = c - floor(c)
//   w >  So: taps j with |j - c| < s, those outside [0, Si - 1] dropped; weight 1 - |j - c| / s, divided by the kept sum
// The two axes decide independently and the pixel is the separable sum: F.interpolate(mode="bilinear", antialias=True,
// align_corners=False) for a whole-image box.  The border is the image edge, not the box edge.
// The coordinate is kept in integers: with D = 2 So and N = w (2 ox' + 1) - So, c = left + N / D, so floor(c) is an integer
// division and every weight is 1 - |D (j - left) - N| / max(2 w, 2 So): one integer-to-float conversion, one product, one
// subtraction.  An output pixel that falls on a source pixel (the identity box, a flip) therefore gets weight 1 exactly and
// the source value bit for bit, for bytes and for floats.
// Streaming, no LDS.  A thread owns 4 adjacent output pixels of one row: the row taps once, the column taps of its 4 pixels
// once (an axis that does not shrink costs the unit ONE integer division: the next pixel's (floor, remainder) is at most one
// wrap away; first two weights in registers: all there is when no axis shrinks, and such a unit runs straight-line code;
// further taps of a shrinking axis are recomputed per row, a 17-entry table per pixel would spill), then every channel with
// them.  Byte images are read through one aligned 8-byte window per row and unit where two taps an axis suffice: one byte
// load per tap is what the older kernel spends its time on.  Stores are packed where the address
// allows: one 32-bit store of 4 bytes, one 16-byte store of 4 floats; the So % 4 tail, and rows that So % 4 != 0 leaves
// unaligned, take one store per pixel.  64-bit offsets, a grid-stride loop under a bounded grid.
// Boxes live on the device and cannot be checked by the launcher: top / left are clamped to [-Si, 2 Si] and h / w to
// [0, 2 Si] (no box inside the image is changed; the integers above then stay below 2^30), every tap index is clamped into
// the image, and a box whose taps all fall outside it takes the nearest pixel: no parameter value reads outside the batch.
#include "kernels.h"

namespace mae {

namespace {

constexpr int RESIZE_MAX_SIZE = 8192;  // in_size and out_size: keeps D (j - left) - N inside an int
constexpr int RESIZE_MAX_RATIO = 8;    // in_size <= 8 out_size: at most 17 taps an axis

// taps lo .. lo + n - 1 of one output pixel on one axis; tap k weighs max(0, 1 - |m0 + k D| inv_g) * scale
struct ResizeAxis {
  int lo, n, m0;
  float scale;
};

__device__ __forceinline__ int floordiv_pos(int a, int d) {  // d > 0
  const int q = a / d;
  return q - (a - q * d < 0);
}
__device__ __forceinline__ float resize_weight(int m, float inv_g) { return fmaxf(1.f - (float)abs(m) * inv_g, 0.f); }

// an axis that keeps or gains pixels, from c = start + q + r / D with 0 <= r < D: the clamped coordinate's two taps
__device__ __forceinline__ ResizeAxis resize_axis_up(int q, int r, int start, int Si) {
  ResizeAxis a;
  a.lo = min(max(start + q, 0), Si - 1); a.n = 1; a.m0 = 0; a.scale = 1.f;   // a clamped coordinate: the nearest pixel, weight 1
  if (start + q >= 0 && start + q < Si - 1 && r != 0) { a.n = 2; a.m0 = -r; }
  return a;
}

// an axis that loses pixels (len > So): the triangle filter of half-width len / So around c = start + N / D.  start / len are
// already clamped to the ranges above
__device__ __forceinline__ ResizeAxis resize_axis_down(int N, int start, int len, int So, int Si, float inv_g) {
  const int D = 2 * So, G = 2 * len;
  ResizeAxis a;
  a.lo = min(max(start + floordiv_pos(N, D), 0), Si - 1); a.n = 1; a.m0 = 0; a.scale = 1.f;   // what an empty tap set takes
  const int jl = max(start + floordiv_pos(N - G, D) + 1, 0), jh = min(start - floordiv_pos(-(N + G), D) - 1, Si - 1);  // |D (j - start) - N| < G
  if (jl > jh) return a;
  const int m0 = D * (jl - start) - N;
  float sum = 0.f;
  for (int k = 0; k <= jh - jl; ++k) sum += resize_weight(m0 + k * D, inv_g);
  if (!(sum > 0.f)) return a;
  a.lo = jl; a.n = jh - jl + 1; a.m0 = m0; a.scale = 1.f / sum;
  return a;
}

// floor(N / D) for N > -D, by one unsigned division
__device__ __forceinline__ int floordiv_above(int N, int D) { return (int)((unsigned)(N + D) / (unsigned)D) - 1; }

__device__ __forceinline__ float resize_px(const uint8_t* p) { return (float)*p; }
__device__ __forceinline__ float resize_px(const float* p) { return *p; }

// unit = 4 adjacent pixels of one output row of one image, every channel; units = B * So * Q, Q = ceil(So / 4)
template <class IN, class OUT>
// at most 4 waves a SIMD: lets the scheduler spend registers on having a unit's loads in flight together (measured: 124 -> 106 us)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 4)))
resize_crop_flip_kernel(const IN* __restrict__ in, const int32_t* __restrict__ params, int64_t units, int C, int Si, int So, int Q,
                        OUT* __restrict__ out, uintptr_t window_end) {
  const uint32_t per = (uint32_t)So * (uint32_t)Q;  // <= 2^24
  const int D = 2 * So;
  for (int64_t u = blockIdx.x * 256ll + threadIdx.x; u < units; u += (int64_t)gridDim.x * 256) {
    const int64_t b = (u >> 32) == 0 ? (int64_t)((uint32_t)u / per) : u / (int64_t)per;
    const uint32_t rem = (uint32_t)(u - b * (int64_t)per);
    const int oy = (int)(rem / (uint32_t)Q), x0 = 4 * (int)(rem - (uint32_t)oy * (uint32_t)Q);
    int top = 0, left = 0, h = Si, w = Si, flip = 0;
    if (params) {
      const int32_t* pb = params + 5 * b;
      top = min(max(pb[0], -Si), 2 * Si); left = min(max(pb[1], -Si), 2 * Si);
      h = min(max(pb[2], 0), 2 * Si); w = min(max(pb[3], 0), 2 * Si);
      flip = pb[4];
    }
    const float igy = 1.f / (float)(2 * max(h, So)), igx = 1.f / (float)(2 * max(w, So));
    const int Ny = h * (2 * oy + 1) - So;   // >= -So
    ResizeAxis ay;
    if (h <= So) { const int q = floordiv_above(Ny, D); ay = resize_axis_up(q, Ny - q * D, top, Si); }
    else ay = resize_axis_down(Ny, top, h, So, Si, igy);
    const float wy0 = resize_weight(ay.m0, igy), wy1 = resize_weight(ay.m0 + D, igy);
    const int npx = min(4, So - x0);
    ResizeAxis ax[4];
    float wx0[4], wx1[4], scale[4];
    const int step = flip ? -2 * w : 2 * w;                              // N of the next output pixel
    const int Nx = w * (2 * (flip ? So - 1 - x0 : x0) + 1) - So;
    bool two = ay.n <= 2;                                                // no axis of this unit takes more than two taps
    if (w <= So) {   // one division for the unit: |step| <= D, so (q, r) of the next pixel is at most one wrap away
      int q = floordiv_above(Nx, D), r = Nx - q * D;
#pragma unroll
      for (int i = 0; i < 4; ++i) {   // a lane past the row's end gets taps clamped like any other and stores nothing
        ax[i] = resize_axis_up(q, r, left, Si);
        r += step;
        const int up = r >= D, dn = r < 0;
        q += up - dn; r += (dn - up) * D;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ax[i] = resize_axis_down(Nx + min(i, npx - 1) * step, left, w, So, Si, igx);   // a lane past the row's end repeats its last pixel
        two = two && ax[i].n <= 2;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      wx0[i] = resize_weight(ax[i].m0, igx);
      wx1[i] = resize_weight(ax[i].m0 + D, igx);
      scale[i] = ax[i].scale * ay.scale;
    }
    // Bytes, two taps an axis: the taps of the unit's four pixels lie within five adjacent bytes of a row (their coordinates are
    // at most one source pixel apart), so ONE aligned 8-byte window per row holds them all -- two 32-bit loads instead of eight
    // byte loads.  window_end (0 = the batch is not 4-byte aligned or not a multiple of 4 bytes long: no windows) is the last
    // address a window may start at, 8 bytes before the end of the batch: a window that would run past it starts there instead
    int sh_a[4], sh_b[4], xmin = 0;
    bool window = false;
    if constexpr (sizeof(IN) == 1) {
      if (two && window_end) {
        xmin = min(min(ax[0].lo, ax[1].lo), min(ax[2].lo, ax[3].lo));
        int xmax = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          sh_a[i] = 8 * (ax[i].lo - xmin); sh_b[i] = sh_a[i] + 8 * (ax[i].n > 1);
          xmax = max(xmax, sh_b[i]);
        }
        window = xmax <= 32;
      }
    }
    for (int c = 0; c < C; ++c) {
      const IN* plane = in + ((int64_t)b * C + c) * Si * Si;
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      if (window) {
        uint64_t win[2];
        int sh[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const uintptr_t a = (uintptr_t)(plane + (int64_t)(ay.lo + (r && ay.n > 1)) * Si + xmin);
          const uintptr_t A = min(a & ~(uintptr_t)3, window_end);
          const uint32_t* wp = reinterpret_cast<const uint32_t*>(A);
          win[r] = (uint64_t)wp[0] | ((uint64_t)wp[1] << 32);
          sh[r] = 8 * (int)(a - A);   // <= 56: the unit's last tap is a byte of the batch, so it lies inside the window wherever it starts
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool tx = ax[i].n > 1;
          const float p00 = (float)(uint32_t)((win[0] >> (sh[0] + sh_a[i])) & 0xff), p01 = (float)(uint32_t)((win[0] >> (sh[0] + sh_b[i])) & 0xff);
          const float p10 = (float)(uint32_t)((win[1] >> (sh[1] + sh_a[i])) & 0xff), p11 = (float)(uint32_t)((win[1] >> (sh[1] + sh_b[i])) & 0xff);
          float rs0 = wx0[i] * p00, rs1 = wx0[i] * p10;
          const float t0 = fmaf(wx1[i], p01, rs0), t1 = fmaf(wx1[i], p11, rs1);
          rs0 = tx ? t0 : rs0; rs1 = tx ? t1 : rs1;
          const float a0 = wy0 * rs0;
          acc[i] = ay.n > 1 ? fmaf(wy1, rs1, a0) : a0;
        }
      } else if (two) {   // straight-line: what every unit of a same-size or growing resize takes.  The same operations in the same order as below
        const IN* row0 = plane + (int64_t)ay.lo * Si;
        const IN* row1 = row0 + (ay.n > 1 ? Si : 0);
        IN raw[4][4];   // all sixteen loads first: nothing below waits for one load at a time
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int xa = ax[i].lo, xb = xa + (ax[i].n > 1);
          raw[i][0] = row0[xa]; raw[i][1] = row0[xb];
          raw[i][2] = row1[xa]; raw[i][3] = row1[xb];
        }
        float p[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int k = 0; k < 4; ++k) p[i][k] = (float)raw[i][k];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool tx = ax[i].n > 1;
          float rs0 = wx0[i] * p[i][0], rs1 = wx0[i] * p[i][2];
          const float t0 = fmaf(wx1[i], p[i][1], rs0), t1 = fmaf(wx1[i], p[i][3], rs1);
          rs0 = tx ? t0 : rs0; rs1 = tx ? t1 : rs1;
          const float a0 = wy0 * rs0;
          acc[i] = ay.n > 1 ? fmaf(wy1, rs1, a0) : a0;
        }
      } else {
        for (int ky = 0; ky < ay.n; ++ky) {
          const float wy = ky == 0 ? wy0 : ky == 1 ? wy1 : resize_weight(ay.m0 + ky * D, igy);
          const IN* row = plane + (int64_t)(ay.lo + ky) * Si;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const IN* p = row + ax[i].lo;
            float rs = wx0[i] * resize_px(p);
            if (ax[i].n > 1) rs = fmaf(wx1[i], resize_px(p + 1), rs);
            for (int kx = 2; kx < ax[i].n; ++kx) rs = fmaf(resize_weight(ax[i].m0 + kx * D, igx), resize_px(p + kx), rs);
            acc[i] = ky == 0 ? wy * rs : fmaf(wy, rs, acc[i]);
          }
        }
      }
      OUT* dst = out + (((int64_t)b * C + c) * So + oy) * So + x0;
      if constexpr (sizeof(IN) == 1) {
        unsigned r[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = (unsigned)(int)fminf(fmaxf(rintf(acc[i] * scale[i]), 0.f), 255.f);
        if constexpr (sizeof(OUT) == 1) {
          if (npx == 4 && ((uintptr_t)dst & 3) == 0) {
            *reinterpret_cast<unsigned*>(dst) = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (i < npx) dst[i] = (uint8_t)r[i];
          }
        } else {
          if (npx == 4 && ((uintptr_t)dst & 15) == 0) {
            store4(dst, f32x4{norm_u8(r[0]), norm_u8(r[1]), norm_u8(r[2]), norm_u8(r[3])});
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (i < npx) dst[i] = norm_u8(r[i]);
          }
        }
      } else {
        if (npx == 4 && ((uintptr_t)dst & 15) == 0) {
          store4(dst, f32x4{acc[0] * scale[0], acc[1] * scale[1], acc[2] * scale[2], acc[3] * scale[3]});
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (i < npx) dst[i] = acc[i] * scale[i];
        }
      }
    }
  }
}

}  // namespace

int launch_resize_crop_flip(const void* images, int in_dt, int B, int C, int Si, const int32_t* params, int So, int out_dt, void* out,
                            hipStream_t s) {
  MAE_REQUIRE(in_dt == MAE_F32 || in_dt == MAE_U8, "resize_crop_flip: in_dtype must be MAE_F32 or MAE_U8 (got %d)", in_dt);
  MAE_REQUIRE(out_dt == MAE_F32 || out_dt == MAE_U8, "resize_crop_flip: out_dtype must be MAE_F32 or MAE_U8 (got %d)", out_dt);
  MAE_REQUIRE(out_dt != MAE_U8 || in_dt == MAE_U8, "resize_crop_flip: uint8 output needs uint8 images (float values have no byte form)");
  MAE_REQUIRE(B > 0 && C > 0 && Si > 0 && So > 0, "resize_crop_flip: bad batch %d / in_chans %d / in_size %d / out_size %d", B, C, Si, So);
  MAE_REQUIRE(Si <= RESIZE_MAX_SIZE && So <= RESIZE_MAX_SIZE, "resize_crop_flip: in_size %d and out_size %d must be <= %d", Si, So,
              RESIZE_MAX_SIZE);
  MAE_REQUIRE(Si <= RESIZE_MAX_RATIO * So, "resize_crop_flip: in_size %d > %d * out_size %d (the tap count is bounded)", Si, RESIZE_MAX_RATIO, So);
  MAE_REQUIRE(images && out, "resize_crop_flip: null images/out");
  const bool in8 = in_dt == MAE_U8, out8 = out_dt == MAE_U8;
  const int64_t in_bytes = (int64_t)B * C * Si * Si * (in8 ? 1 : 4), out_bytes = (int64_t)B * C * So * So * (out8 ? 1 : 4);
  MAE_REQUIRE(!((uintptr_t)out < (uintptr_t)images + (uintptr_t)in_bytes && (uintptr_t)images < (uintptr_t)out + (uintptr_t)out_bytes),
              "resize_crop_flip: out may not overlap images (an output pixel reads several source pixels)");
  MAE_REQUIRE((in8 || ((uintptr_t)images & 3) == 0) && (out8 || ((uintptr_t)out & 3) == 0) && ((uintptr_t)params & 3) == 0,
              "resize_crop_flip: float buffers and params must be 4-byte aligned");
  const int Q = (So + 3) / 4;
  const int64_t units = (int64_t)B * So * Q;
  const dim3 grid((unsigned)std::min<int64_t>(cdiv(units, 256), 256 * 32));
  // 8-byte windows over a byte batch: only where every aligned window lies inside it (see the kernel)
  const uintptr_t window_end = in8 && ((uintptr_t)images & 3) == 0 && in_bytes % 4 == 0 && in_bytes >= 8 ? (uintptr_t)images + (uintptr_t)in_bytes - 8 : 0;
#define RESIZE(IN, OUT) \
  hipLaunchKernelGGL((resize_crop_flip_kernel<IN, OUT>), grid, dim3(256), 0, s, (const IN*)images, params, units, C, Si, So, Q, (OUT*)out, \
                     window_end)
  if (in8 && out8) RESIZE(uint8_t, uint8_t);
  else if (in8) RESIZE(uint8_t, float);
  else RESIZE(float, float);
#undef RESIZE
  MAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace mae

extern "C" int mae_resize_crop_flip(const void* images, int32_t in_dtype, int32_t batch, int32_t in_chans, int32_t in_size, const int32_t* params,
                                    int32_t out_size, int32_t out_dtype, void* out, void* stream) {
  return mae::launch_resize_crop_flip(images, in_dtype, batch, in_chans, in_size, params, out_size, out_dtype, out, (hipStream_t)stream);
}
