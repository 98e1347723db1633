// Batch mixing for classifier fine-tuning: mixup (Zhang et al. 2018) and CutMix (Yun et al. 2019) as timm's Mixup applies them
// in `batch` mode -- image b is mixed with image partner[b] of the same batch:
//   inside  box[b] = (y0, y1, x0, x1), half-open, clamped to [0, S]:  out = n(partner pixel)
//   outside                                                        :  out = lam[b] * n(own) + (1 - lam[b]) * n(partner)
// n() is norm_u8 for uint8 images (the expression every pixel kernel of the engine uses: bit-identical to them) and the identity
// for fp32 ones.  lam[b] == 1 copies n(own) bit for bit.  With uint8 output (pure CutMix) nothing is normalised and lam is not
// read: the partner's byte inside the box, the own byte outside, so the batch stays 1 byte per pixel for the engine.
// Data movement only.  A thread owns V contiguous pixels of one row, 16 bytes of the output when the row length allows: V = 4
// for fp32 output (one 16-byte store per lane, contiguous across the wave; the uint8 input is then a 4-byte load), V = 16 for
// uint8 output (16-byte loads and stores); V = 4 / 1 for other row lengths.  16 uint8 pixels per thread with fp32 output would
// make each lane issue four 16-byte stores 64 bytes apart, which is no faster than the contiguous store; 4 pixels per thread
// with uint8 output halves the rate (profiles/README.md, r14).  The box edges are a per-pixel select.  A vector wholly inside the box never loads the own image, one wholly outside it with nothing to blend never loads
// the partner.
#include "kernels.h"

namespace mae {

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// V raw pixels of one row: bytes as unsigned, floats as they are
template <int V> __device__ __forceinline__ void mix_load(const uint8_t* __restrict__ p, unsigned (&o)[V]) {
  if constexpr (V == 16) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = (w[i / 4] >> (8 * (i % 4))) & 0xff;
  } else if constexpr (V == 4) {
    const unsigned w = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (w >> (8 * i)) & 0xff;
  } else {
    o[0] = p[0];
  }
}
template <int V> __device__ __forceinline__ void mix_load(const float* __restrict__ p, float (&o)[V]) {
  static_assert(V == 4 || V == 1, "fp32 rows move 16 or 4 bytes per thread");
  if constexpr (V == 4) { const f32x4 v = load4(p); o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3]; }
  else o[0] = p[0];
}
template <int V> __device__ __forceinline__ void mix_store(uint8_t* __restrict__ p, const unsigned (&v)[V]) {
  if constexpr (V == 16) {
    u32x4 w;
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = v[4 * q] | (v[4 * q + 1] << 8) | (v[4 * q + 2] << 16) | (v[4 * q + 3] << 24);
    *reinterpret_cast<u32x4*>(p) = w;
  } else if constexpr (V == 4) {
    *reinterpret_cast<unsigned*>(p) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
  } else {
    p[0] = (uint8_t)v[0];
  }
}
template <int V> __device__ __forceinline__ void mix_store(float* __restrict__ p, const float (&v)[V]) {
  static_assert(V == 4 || V == 1, "fp32 rows move 16 or 4 bytes per thread");
  if constexpr (V == 4) store4(p, f32x4{v[0], v[1], v[2], v[3]});
  else p[0] = v[0];
}
__device__ __forceinline__ float mix_norm(unsigned u) { return norm_u8(u); }
__device__ __forceinline__ float mix_norm(float v) { return v; }

template <class T> struct MixRaw { typedef float type; };
template <> struct MixRaw<uint8_t> { typedef unsigned type; };

// unit = V pixels of one row of one plane; units = B * C * S * (S / V) <= 2^31 - 256 (checked by the launcher)
template <class IN, class OUT, int V>
__global__ void __launch_bounds__(256) mix_batch_kernel(const IN* __restrict__ images, const int32_t* __restrict__ partner,
                                                        const float* __restrict__ lam, const int32_t* __restrict__ box, int units, int B, int C,
                                                        int S, OUT* __restrict__ out) {
  typedef typename MixRaw<IN>::type raw_t;
  typedef typename MixRaw<OUT>::type res_t;
  constexpr bool BYTES = sizeof(OUT) == 1;  // pure CutMix on raw bytes
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= units) return;
  const int sv = S / V;
  const int row = (int)((uint32_t)u / (uint32_t)sv), x = (u - row * sv) * V;   // row = (b * C + c) * S + y
  const int bc = (int)((uint32_t)row / (uint32_t)S), y = row - bc * S;
  const int b = (int)((uint32_t)bc / (uint32_t)C), c = bc - b * C;
  const int pb_raw = partner[b];
  const int pb = (pb_raw >= 0 && pb_raw < B) ? pb_raw : b;  // an out-of-range partner is never an index: the image mixes with itself
  const int y0 = min(max(box[4 * b], 0), S), y1 = min(max(box[4 * b + 1], 0), S);
  const int x0 = min(max(box[4 * b + 2], 0), S), x1 = min(max(box[4 * b + 3], 0), S);
  const bool row_in = y >= y0 && y < y1;
  const bool any_in = row_in && x < x1 && x + V > x0;
  const bool all_in = row_in && x >= x0 && x + V <= x1;
  float l = 1.f;
  if constexpr (!BYTES) l = lam[b];
  const int64_t own_off = (int64_t)row * S + x;
  const int64_t par_off = ((int64_t)(pb * C + c) * S + y) * S + x;
  raw_t a[V], p[V];
#pragma unroll
  for (int i = 0; i < V; ++i) { a[i] = 0; p[i] = 0; }
  if (!all_in) mix_load<V>(images + own_off, a);
  if (any_in || (!BYTES && l != 1.f)) mix_load<V>(images + par_off, p);
  res_t r[V];
  const float lb = 1.f - l;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const bool in = row_in && x + i >= x0 && x + i < x1;
    if constexpr (BYTES) {
      r[i] = in ? p[i] : a[i];
    } else {
      const float na = mix_norm(a[i]), np = mix_norm(p[i]);
      r[i] = in ? np : (l == 1.f ? na : l * na + lb * np);
    }
  }
  mix_store<V>(out + own_off, r);
}

}  // namespace

int launch_mix_batch(const void* images, int img_dt, const int32_t* partner, const float* lam, const int32_t* box, int B, int C, int S,
                     int out_dt, void* out, hipStream_t s) {
  MAE_REQUIRE(img_dt == MAE_F32 || img_dt == MAE_U8, "mix_batch: image_dtype must be MAE_F32 or MAE_U8 (got %d)", img_dt);
  MAE_REQUIRE(out_dt == MAE_F32 || out_dt == MAE_U8, "mix_batch: out_dtype must be MAE_F32 or MAE_U8 (got %d)", out_dt);
  MAE_REQUIRE(out_dt != MAE_U8 || img_dt == MAE_U8, "mix_batch: uint8 output (pure CutMix) needs uint8 images");
  MAE_REQUIRE(B > 0 && C > 0 && S > 0 && S <= 16384, "mix_batch: bad batch %d / in_chans %d / image_size %d", B, C, S);
  MAE_REQUIRE(images && partner && box && out && (lam || out_dt == MAE_U8), "mix_batch: null images/partner/lam/box/out");
  const bool in8 = img_dt == MAE_U8, out8 = out_dt == MAE_U8;
  // pixels per thread: 16 bytes of the OUTPUT where the row length allows it (fp32: 4 pixels, uint8: 16)
  const int V = out8 && S % 16 == 0 ? 16 : S % 4 == 0 ? 4 : 1;
  const int64_t px = (int64_t)B * C * S * S, units = px / V;
  MAE_REQUIRE(units <= (1ll << 31) - 256, "mix_batch: batch * in_chans * image_size^2 / %d must be <= 2^31 - 256", V);  // blockIdx * 256 + t stays an int
  const int64_t in_bytes = px * (in8 ? 1 : 4), out_bytes = px * (out8 ? 1 : 4);
  MAE_REQUIRE(!((uintptr_t)out < (uintptr_t)images + (uintptr_t)in_bytes && (uintptr_t)images < (uintptr_t)out + (uintptr_t)out_bytes),
              "mix_batch: out may not overlap images (a mixed pixel reads two images)");
  const uintptr_t in_align = in8 ? V : 4 * V, out_align = out8 ? V : 4 * V;
  MAE_REQUIRE(((uintptr_t)images & (in_align - 1)) == 0 && ((uintptr_t)out & (out_align - 1)) == 0 && ((uintptr_t)partner & 3) == 0 &&
                  ((uintptr_t)box & 3) == 0 && ((uintptr_t)lam & 3) == 0,
              "mix_batch: images must be %d-byte and out %d-byte aligned for image_size %d; partner / lam / box 4-byte", (int)in_align,
              (int)out_align, S);
  const dim3 grid((unsigned)cdiv(units, 256));
#define MIX(IN, OUT, V) \
  hipLaunchKernelGGL((mix_batch_kernel<IN, OUT, V>), grid, dim3(256), 0, s, (const IN*)images, partner, lam, box, (int)units, B, C, S, (OUT*)out)
  if (in8 && out8) { if (V == 16) MIX(uint8_t, uint8_t, 16); else if (V == 4) MIX(uint8_t, uint8_t, 4); else MIX(uint8_t, uint8_t, 1); }
  else if (in8)    { if (V == 4) MIX(uint8_t, float, 4); else MIX(uint8_t, float, 1); }
  else             { if (V == 4) MIX(float, float, 4); else MIX(float, float, 1); }
#undef MIX
  MAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace mae

extern "C" int mae_mix_batch(const void* images, int32_t image_dtype, const int32_t* partner, const float* lam, const int32_t* box,
                             int32_t batch, int32_t in_chans, int32_t image_size, int32_t out_dtype, void* out, void* stream) {
  return mae::launch_mix_batch(images, image_dtype, partner, lam, box, batch, in_chans, image_size, out_dtype, out, (hipStream_t)stream);
}
