// Per-image augmentation of the classifier fine-tuning recipe (MAE / BEiT / DeiT): RandomResizedCrop + flip, RandAugment
// and random erasing on uint8 images, with the semantics of the PIL calls timm makes, per element.
//
// One workgroup (512 threads) owns one image.  The whole image (C planes of S x S bytes) lives in LDS in two ping-pong buffers, beside a
// 3 x 256 table of words (histogram, then lookup table) and a few scalars:
//   [ buffer 0: C S S bytes, padded to 16 ][ buffer 1: the same ][ table: 768 words ][ scalars: 32 words ]
// Every op reads one buffer and writes the other, so op k + 1 sees the rounded uint8 result of op k, which is how a chain of
// PIL transforms behaves; an op that does nothing (NONE, an unknown id) leaves the buffers as they are.  The image is read
// from memory once and written once, whatever the number of ops.  2 C S S + 3200 bytes must fit the 160 KiB of a CU's LDS:
// S <= 160 at C = 3 (the launcher refuses larger images before launching).
//
// Arithmetic is the one PIL's C code has, so that the bytes are PIL's: integer point ops and tables; the ImageEnhance blends
// in fp32 with the product and the sum rounded separately; the autocontrast table and the affine map in fp64, again every
// operation rounded on its own.  That needs UNFUSED multiply-adds, and this toolchain fuses them under the library's
// -ffp-contract=fast whatever the source says (a file-scope contract pragma and the __dmul_rn family are both fused):
// the Makefile therefore appends -ffp-contract=off to THIS object's command line, and to no other.
//
// Rule for images that are not RGB: every op except AFFINE reads or defines colour, so with in_chans != 3 the launcher
// refuses num_ops > 0 unless the caller states, with MAE_AUG_GEOMETRIC in out_dtype, that it sends AFFINE / NONE only; the
// kernel then treats every other id as NONE (an id is never trusted, and never used as an index).
//
// Erasing (timm RandomErasing, `pixel` mode) and the output conversion run last: MAE_F32 output is norm_u8(byte), and the
// elements inside the image's erase box are N(0, 1) noise from a counter-based generator, so a reference can reproduce it:
//   e = (c S + y) S + x, w0 = mix(seed, 2e), w1 = mix(seed, 2e + 1), mix(s, i) = fmix32(fmix32(i + 0x9E3779B9) ^ s),
//   u1 = ((w0 >> 8) + 1) 2^-24, u2 = (w1 >> 8) 2^-24, n = sqrtf(-2 logf(u1)) cosf(2 pi u2).
#include "kernels.h"

namespace mae {

namespace {

constexpr int AUG_THREADS = 512;   // two workgroups of 8 waves per CU at 96 px: 0.46 ms for the recipe at B = 2000 against 0.58 (256 threads) and 0.53 (1024)
static_assert(AUG_THREADS >= 256 && AUG_THREADS % 64 == 0 && AUG_THREADS <= 1024, "the table ops give one histogram bin to each of the first 256 threads");
constexpr int AUG_MAX_OPS = 8;
constexpr int AUG_TABLE_WORDS = 3 * 256;
constexpr int AUG_SCALAR_WORDS = 32;
constexpr int AUG_LDS_LIMIT = 160 * 1024;
constexpr int AUG_FLAG_MASK = MAE_AUG_GEOMETRIC;

// Image.blend(degenerate, image, alpha): fp32, product and sum rounded separately (this file is built with contraction off)
__device__ __forceinline__ unsigned aug_blend(int d, int v, float alpha, bool unit) {
  const float t = (float)d + alpha * (float)(v - d);
  if (unit) return (unsigned)(int)t;   // 0 <= alpha <= 1: t lies between d and v
  return t <= 0.f ? 0u : t >= 255.f ? 255u : (unsigned)(int)t;
}

// ImageMode L of an RGB pixel
__device__ __forceinline__ int aug_lum(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// fmix32 / aug_mix: common.cuh (shared with k_umap.hip)
__device__ __forceinline__ float aug_noise(uint32_t seed, uint32_t e) {
  const uint32_t w0 = aug_mix(seed, 2u * e), w1 = aug_mix(seed, 2u * e + 1u);
  const float u1 = (float)((w0 >> 8) + 1u) * 0x1p-24f, u2 = (float)(w1 >> 8) * 0x1p-24f;
  return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// a byte-wise map of the whole image, four bytes per step (the buffers are padded to whole words)
template <class F>
__device__ __forceinline__ void aug_point(const uint8_t* cur, uint8_t* nxt, int n, F f) {
  const unsigned* s = reinterpret_cast<const unsigned*>(cur);
  unsigned* d = reinterpret_cast<unsigned*>(nxt);
  for (int w = threadIdx.x; w < (n + 3) / 4; w += AUG_THREADS) {
    const unsigned v = s[w];
    d[w] = f(v & 0xff) | (f((v >> 8) & 0xff) << 8) | (f((v >> 16) & 0xff) << 16) | (f(v >> 24) << 24);
  }
}

// PIL's BICUBIC macro (Geometry.c), Horner form
__device__ __forceinline__ double aug_cubic(double v1, double v2, double v3, double v4, double d) {
  const double p1 = v2;
  const double p2 = -v1 + v3;
  const double p3 = 2 * (v1 - v2) + v3 - v4;
  const double p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

// Image.transform(AFFINE, m, resample, fillcolor): output pixel centres mapped by m in fp64; a centre that leaves [0, S) takes the fill
__device__ void aug_affine(const uint8_t* cur, uint8_t* nxt, int C, int S, const double* __restrict__ m, int iarg) {
  const int mode = iarg & 0xff, fill = (iarg >> 8) & 0xffffff, plane = S * S;
  const bool linear = mode == 0 || mode == 2;
  const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
  for (int p = threadIdx.x; p < plane; p += AUG_THREADS) {
    const int oy = p / S, ox = p - oy * S;
    const double cx = (double)ox + 0.5, cy = (double)oy + 0.5;
    double xin = m0 * cx + m1 * cy + m2;
    double yin = m3 * cx + m4 * cy + m5;
    if (!(xin >= 0.0 && xin < (double)S && yin >= 0.0 && yin < (double)S)) {   // PIL's test; a NaN coordinate counts as outside
      for (int c = 0; c < C; ++c) nxt[c * plane + p] = (uint8_t)(C == 3 ? (fill >> (8 * (2 - c))) & 0xff : fill & 0xff);
      continue;
    }
    xin -= 0.5; yin -= 0.5;
    const double fx = floor(xin), fy = floor(yin);
    const int x = (int)fx, y = (int)fy;
    const double dx = xin - fx, dy = yin - fy;
    int xs[4], ys[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { xs[k] = min(max(x - 1 + k, 0), S - 1); ys[k] = min(max(y - 1 + k, 0), S - 1) * S; }
    for (int c = 0; c < C; ++c) {
      const uint8_t* pc = cur + c * plane;
      double v;
      if (linear) {
        const double a0 = (double)pc[ys[1] + xs[1]], b0 = (double)pc[ys[1] + xs[2]];
        const double a1 = (double)pc[ys[2] + xs[1]], b1 = (double)pc[ys[2] + xs[2]];
        const double v1 = a0 + (b0 - a0) * dx, v2 = a1 + (b1 - a1) * dx;
        v = v1 + (v2 - v1) * dy;
      } else {
        double r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          r[k] = aug_cubic((double)pc[ys[k] + xs[0]], (double)pc[ys[k] + xs[1]], (double)pc[ys[k] + xs[2]], (double)pc[ys[k] + xs[3]], dx);
        v = aug_cubic(r[0], r[1], r[2], r[3], dy);
      }
      int q;
      if (mode == 0) q = (int)v;
      else if (v <= 0.0) q = 0;
      else if (v >= 255.0) q = 255;
      else q = mode == 1 ? (int)v : (int)floor(v + 0.5);
      nxt[c * plane + p] = (uint8_t)q;
    }
  }
}

// ImageOps.autocontrast / equalize of an RGB image: per channel a histogram, a 256-entry table, a lookup.  The first 256 threads own one bin each.
__device__ void aug_table_op(const uint8_t* cur, uint8_t* nxt, int S, bool equalize, int* tab, int* sc) {
  const int plane = S * S, t = threadIdx.x;
  for (int i = t; i < AUG_TABLE_WORDS; i += AUG_THREADS) tab[i] = 0;
  if (t < 3) { sc[4 * t] = 256; sc[4 * t + 1] = -1; sc[4 * t + 2] = 0; }
  __syncthreads();
  for (int c = 0; c < 3; ++c)
    for (int p = t; p < plane; p += AUG_THREADS) atomicAdd(&tab[c * 256 + cur[c * plane + p]], 1);
  __syncthreads();
  int h[3] = {0, 0, 0}, incl[3] = {0, 0, 0}, lut[3] = {0, 0, 0};
  if (t < 256) {   // the first four waves, whole: one bin per thread
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      h[c] = tab[c * 256 + t];
      if (h[c] > 0) { atomicMin(&sc[4 * c], t); atomicMax(&sc[4 * c + 1], t); atomicAdd(&sc[4 * c + 2], 1); }
      int v = h[c];   // inclusive scan over the wave's 64 bins; the wave totals go through LDS
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o, 64); if ((t & 63) >= o) v += u; }
      incl[c] = v;
      if ((t & 63) == 63) sc[12 + 4 * c + (t >> 6)] = v;
    }
  }
  __syncthreads();
  if (t < 256) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int lo = sc[4 * c], hi = sc[4 * c + 1], nnz = sc[4 * c + 2];
      lut[c] = t;
      if (equalize) {
        int before = incl[c] - h[c];
        for (int w = 0; w < (t >> 6); ++w) before += sc[12 + 4 * c + w];
        const int step = nnz > 1 ? (plane - tab[c * 256 + hi]) / 255 : 0;   // sum of the non-zero bins less the last of them
        if (step > 0) lut[c] = min(255, (step / 2 + before) / step);
      } else if (hi > lo) {
        const double scale = 255.0 / (double)(hi - lo);
        const double off = (double)(-lo) * scale;
        const int q = (int)((double)t * scale + off);
        lut[c] = min(max(q, 0), 255);
      }
    }
  }
  __syncthreads();   // every read of the histogram is done: the table takes its place
  if (t < 256) {
#pragma unroll
    for (int c = 0; c < 3; ++c) tab[c * 256 + t] = lut[c];
  }
  __syncthreads();
  for (int c = 0; c < 3; ++c)
    for (int p = t; p < plane; p += AUG_THREADS) nxt[c * plane + p] = (uint8_t)tab[c * 256 + cur[c * plane + p]];
}

template <class OUT>
__global__ void __launch_bounds__(AUG_THREADS) augment_ops_u8_kernel(const uint8_t* __restrict__ images, int C, int S, const int32_t* __restrict__ op_codes,
                                                             const double* __restrict__ op_args, int num_ops, const int32_t* __restrict__ erase,
                                                             int geometric, OUT* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned lds32[];
  constexpr bool F32 = sizeof(OUT) == 4;
  const int plane = S * S, n = C * plane, buf_bytes = (n + 15) & ~15, t = threadIdx.x;
  uint8_t* cur = reinterpret_cast<uint8_t*>(lds32);
  uint8_t* nxt = cur + buf_bytes;
  int* tab = reinterpret_cast<int*>(cur + 2 * buf_bytes);
  int* sc = tab + AUG_TABLE_WORDS;
  const int64_t b = blockIdx.x;
  const uint8_t* src = images + b * n;
  if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0) {
    const unsigned* s32 = reinterpret_cast<const unsigned*>(src);
    for (int w = t; w < n / 4; w += AUG_THREADS) lds32[w] = s32[w];
  } else {
    for (int i = t; i < n; i += AUG_THREADS) cur[i] = src[i];
  }
  __syncthreads();

  for (int k = 0; k < num_ops; ++k) {
    const int32_t* oc = op_codes + (b * num_ops + k) * 2;
    int code = __builtin_amdgcn_readfirstlane(oc[0]);
    const int iarg = __builtin_amdgcn_readfirstlane(oc[1]);
    const double* a = op_args + (b * num_ops + k) * 6;
    if (code < MAE_AUG_NONE || code > MAE_AUG_AFFINE) code = MAE_AUG_NONE;   // an id is never an index
    if ((C != 3 || geometric) && code != MAE_AUG_AFFINE) code = MAE_AUG_NONE;
    if (code == MAE_AUG_NONE) continue;
    const float f = (float)a[0];
    const bool unit = f >= 0.f && f <= 1.f;
    switch (code) {
      case MAE_AUG_INVERT: aug_point(cur, nxt, n, [](unsigned v) { return 255u - v; }); break;
      case MAE_AUG_SOLARIZE: aug_point(cur, nxt, n, [iarg](unsigned v) { return (int)v < iarg ? v : 255u - v; }); break;
      case MAE_AUG_SOLARIZE_ADD: aug_point(cur, nxt, n, [iarg](unsigned v) { return v < 128u ? (unsigned)min(255, max(0, (int)v + iarg)) : v; }); break;
      case MAE_AUG_POSTERIZE: {
        const unsigned mask = iarg >= 8 ? 0xffu : iarg <= 0 ? 0u : (~((1u << (8 - iarg)) - 1u)) & 0xffu;
        aug_point(cur, nxt, n, [mask](unsigned v) { return v & mask; });
      } break;
      case MAE_AUG_BRIGHTNESS: aug_point(cur, nxt, n, [f, unit](unsigned v) { return aug_blend(0, (int)v, f, unit); }); break;
      case MAE_AUG_AUTOCONTRAST: aug_table_op(cur, nxt, S, false, tab, sc); break;
      case MAE_AUG_EQUALIZE: aug_table_op(cur, nxt, S, true, tab, sc); break;
      case MAE_AUG_COLOR:
        for (int p = t; p < plane; p += AUG_THREADS) {
          const int r = cur[p], g = cur[plane + p], bl = cur[2 * plane + p], d = aug_lum(r, g, bl);
          nxt[p] = (uint8_t)aug_blend(d, r, f, unit);
          nxt[plane + p] = (uint8_t)aug_blend(d, g, f, unit);
          nxt[2 * plane + p] = (uint8_t)aug_blend(d, bl, f, unit);
        }
        break;
      case MAE_AUG_CONTRAST: {   // the degenerate image is the rounded mean luminance (ImageStat mean of the L image)
        if (t == 0) sc[0] = 0;
        __syncthreads();
        int sum = 0;   // <= 255 S^2 < 2^31
        for (int p = t; p < plane; p += AUG_THREADS) sum += aug_lum(cur[p], cur[plane + p], cur[2 * plane + p]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if ((t & 63) == 0) atomicAdd(&sc[0], sum);
        __syncthreads();
        const int d = (int)((double)sc[0] / (double)plane + 0.5);
        aug_point(cur, nxt, n, [d, f, unit](unsigned v) { return aug_blend(d, (int)v, f, unit); });
      } break;
      case MAE_AUG_SHARPNESS:   // the degenerate image is ImageFilter.SMOOTH: (1 1 1 / 1 5 1 / 1 1 1) / 13, border = source
        for (int i = t; i < n; i += AUG_THREADS) {
          const int c = i / plane, p = i - c * plane, y = p / S, x = p - y * S;
          const int v = cur[i];
          int d = v;
          if (y > 0 && y < S - 1 && x > 0 && x < S - 1) {
            const uint8_t* q = cur + i;
            const int s = q[-S - 1] + q[-S] + q[-S + 1] + q[-1] + 5 * v + q[1] + q[S - 1] + q[S] + q[S + 1];
            d = (2 * s + 13) / 26;
          }
          nxt[i] = (uint8_t)aug_blend(d, v, f, unit);
        }
        break;
      default: aug_affine(cur, nxt, C, S, a, iarg); break;   // MAE_AUG_AFFINE
    }
    __syncthreads();
    uint8_t* sw = cur; cur = nxt; nxt = sw;
  }

  // erase box (fp32 output only), clamped here; an empty or inverted box erases nothing
  int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
  uint32_t seed = 0;
  if (F32 && erase) {
    const int32_t* e = erase + b * 5;
    y0 = min(max(e[0], 0), S); y1 = min(max(e[1], 0), S); x0 = min(max(e[2], 0), S); x1 = min(max(e[3], 0), S);
    seed = (uint32_t)e[4];
  }
  const bool boxed = y0 < y1 && x0 < x1;
  OUT* dst = out + b * n;
  if constexpr (F32) {
    auto value = [&](int i) -> float {
      if (boxed) {
        const int r = i / S, x = i - r * S, y = r % S;   // r = c S + y
        if (y >= y0 && y < y1 && x >= x0 && x < x1) return aug_noise(seed, (uint32_t)i);
      }
      return norm_u8(cur[i]);
    };
    if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
      for (int w = t; w < n / 4; w += AUG_THREADS) store4(dst + 4 * w, f32x4{value(4 * w), value(4 * w + 1), value(4 * w + 2), value(4 * w + 3)});
    } else {
      for (int i = t; i < n; i += AUG_THREADS) dst[i] = value(i);
    }
  } else {
    if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
      const unsigned* c32 = reinterpret_cast<const unsigned*>(cur);
      for (int w = t; w < n / 4; w += AUG_THREADS) reinterpret_cast<unsigned*>(dst)[w] = c32[w];
    } else {
      for (int i = t; i < n; i += AUG_THREADS) dst[i] = cur[i];
    }
  }
}

}  // namespace

int launch_augment_ops_u8(const uint8_t* images, int B, int C, int S, const int32_t* op_codes, const double* op_args, int num_ops,
                          const int32_t* erase, int out_dt_flags, void* out, hipStream_t s) {
  const int out_dt = out_dt_flags & ~AUG_FLAG_MASK;
  const bool geometric = (out_dt_flags & MAE_AUG_GEOMETRIC) != 0;
  MAE_REQUIRE(out_dt == MAE_F32 || out_dt == MAE_U8, "augment_ops_u8: out_dtype must be MAE_F32 or MAE_U8, optionally with MAE_AUG_GEOMETRIC (got %d)", out_dt_flags);
  MAE_REQUIRE(images && out, "augment_ops_u8: null images / out");
  MAE_REQUIRE(B > 0 && C > 0 && S > 0, "augment_ops_u8: bad batch %d / in_chans %d / image_size %d", B, C, S);
  MAE_REQUIRE(num_ops >= 0 && num_ops <= AUG_MAX_OPS, "augment_ops_u8: num_ops must be in 0..%d (got %d)", AUG_MAX_OPS, num_ops);
  MAE_REQUIRE(num_ops == 0 || (op_codes && op_args), "augment_ops_u8: null op_codes / op_args with num_ops %d", num_ops);
  MAE_REQUIRE(num_ops == 0 || C == 3 || geometric,
              "augment_ops_u8: colour ops need in_chans == 3 (got %d); pass MAE_AUG_GEOMETRIC in out_dtype when every op is AFFINE or NONE", C);
  const int64_t n = (int64_t)C * S * S, buf = (n + 15) & ~(int64_t)15;
  const int64_t lds = 2 * buf + 4 * (AUG_TABLE_WORDS + AUG_SCALAR_WORDS);
  MAE_REQUIRE(S <= 16384 && C <= 16384 && lds <= AUG_LDS_LIMIT,
              "augment_ops_u8: two copies of an image (%d x %d x %d bytes) and the tables need %lld bytes of LDS, more than the %d of a CU "
              "(image_size <= 160 at 3 channels)", C, S, S, (long long)lds, AUG_LDS_LIMIT);
  const int64_t in_bytes = (int64_t)B * n, out_bytes = in_bytes * (out_dt == MAE_U8 ? 1 : 4);
  MAE_REQUIRE(!((uintptr_t)out < (uintptr_t)images + (uintptr_t)in_bytes && (uintptr_t)images < (uintptr_t)out + (uintptr_t)out_bytes),
              "augment_ops_u8: out may not be or overlap images");
  MAE_REQUIRE(((uintptr_t)op_codes & 3) == 0 && ((uintptr_t)op_args & 7) == 0 && ((uintptr_t)erase & 3) == 0 &&
                  (out_dt == MAE_U8 || ((uintptr_t)out & 3) == 0),
              "augment_ops_u8: op_codes / erase must be 4-byte, op_args 8-byte and an fp32 out 4-byte aligned");
  if (lds > 64 * 1024) {   // beyond what a kernel gets by default
    MAE_HIP(hipFuncSetAttribute((const void*)augment_ops_u8_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    MAE_HIP(hipFuncSetAttribute((const void*)augment_ops_u8_kernel<uint8_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  if (out_dt == MAE_F32)
    hipLaunchKernelGGL((augment_ops_u8_kernel<float>), dim3((unsigned)B), dim3(AUG_THREADS), (size_t)lds, s, images, C, S, op_codes, op_args, num_ops, erase,
                       (int)geometric, (float*)out);
  else
    hipLaunchKernelGGL((augment_ops_u8_kernel<uint8_t>), dim3((unsigned)B), dim3(AUG_THREADS), (size_t)lds, s, images, C, S, op_codes, op_args, num_ops,
                       (const int32_t*)nullptr, (int)geometric, (uint8_t*)out);
  MAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace mae

extern "C" int mae_augment_ops_u8(const uint8_t* images, int32_t batch, int32_t in_chans, int32_t image_size, const int32_t* op_codes,
                                  const double* op_args, int32_t num_ops, const int32_t* erase, int32_t out_dtype, void* out, void* stream) {
  return mae::launch_augment_ops_u8(images, batch, in_chans, image_size, op_codes, op_args, num_ops, erase, out_dtype, out, (hipStream_t)stream);
}
