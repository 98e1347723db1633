// Token-row data movement: token assembly (cls / position table), decoder scatter with mask tokens, and their adjoints.  All
// HBM-bound.  (The kernels that read the image -- gather_patches, patchify_gather, the pixel loss -- are in k_pixels.hip.)
// Reference behaviour:
//   gather_patches + patch GEMM + assemble_visible == timm PatchEmbed conv (k = s = patch) -> cat(cls) -> +pos_embed
//     -> gather(idx_keep)           (lightly MaskedVisionTransformerTIMM.preprocess, via src/models/mae.py:55)
//   decoder_assemble == repeat_token(mask_token) -> set_at_index(idx_keep, x_decode) -> + decoder_pos_embed
//                                   (src/models/mae.py:61-71)
#include "kernels.h"

namespace mae {

// x[r] = (t == 0 ? cls : x[r]) + pos[t], fp32 in place, D % 4 == 0
__global__ void __launch_bounds__(256) assemble_visible_kernel(float* __restrict__ x, const int32_t* __restrict__ tok,
                                                               const float* __restrict__ cls,
                                                               const float* __restrict__ pos, int64_t rows, int D4) {
  const int64_t total = rows * D4;
  for (int64_t u = blockIdx.x * 256ll + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const int64_t r = u / D4;
    const int d = (int)(u - r * D4) * 4;
    const int t = tok[r];
    float* px = x + r * (int64_t)D4 * 4 + d;
    f32x4 v = (t == 0) ? load4(cls + d) : load4(px);
    v += load4(pos + (int64_t)t * D4 * 4 + d);
    store4(px, v);
  }
}

int launch_assemble_visible(float* x, const int32_t* tok, const float* cls, const float* pos, int64_t rows, int D,
                            hipStream_t s) {
  MAE_REQUIRE(x && tok && cls && pos && rows > 0 && D % 4 == 0, "assemble_visible: bad arguments (D %% 4 must be 0)");
  const int grid = (int)std::min<int64_t>(cdiv(rows * (D / 4), 256), 256 * 16);
  hipLaunchKernelGGL(assemble_visible_kernel, dim3(grid), dim3(256), 0, s, x, tok, cls, pos, rows, D / 4);
  MAE_LAUNCH_CHECK();
  return 0;
}

// Second stage of every two-stage column reduction: 32 columns per block (8 lanes x float4), 32 row lanes, fixed order.
__device__ __forceinline__ void sum_partials_block(const float* __restrict__ partial, int G, int C, float* __restrict__ out0,
                                                   float* __restrict__ out1, int split, int blk) {
  __shared__ __attribute__((aligned(16))) float red[32][36];
  const int cl = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int c = blk * 32 + cl * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (c < C)
    for (int i = rl; i < G; i += 32) acc += load4(partial + (int64_t)i * C + c);
  store4(&red[rl][cl * 4], acc);
  __syncthreads();
  if (threadIdx.x < 32) {
    const int cc = blk * 32 + threadIdx.x;
    if (cc < C) {
      float v = 0.f;
#pragma unroll
      for (int j = 0; j < 32; ++j) v += red[j][threadIdx.x];
      if (cc < split) out0[cc] = v; else out1[cc - split] = v;
    }
  }
}

__global__ void __launch_bounds__(256) sum_partials_kernel(const float* __restrict__ partial, int G, int C,
                                                           float* __restrict__ out0, float* __restrict__ out1, int split) {
  sum_partials_block(partial, G, C, out0, out1, split, blockIdx.x);
}

// the same for a table of reductions: block -> (entry, 32-column group)
__global__ void __launch_bounds__(256) sum_partials_many_kernel(const PartialsTable tab) {
  int e = 0;
  while (e + 1 < tab.n && (int)blockIdx.x >= tab.block_begin[e + 1]) ++e;
  sum_partials_block(tab.partial[e], tab.G[e], tab.C[e], tab.out0[e], tab.out1[e], tab.split[e], blockIdx.x - tab.block_begin[e]);
}

int launch_sum_partials_many(const PartialsTable& tab, hipStream_t s) {
  if (tab.n == 0) return 0;
  MAE_REQUIRE(tab.n <= PartialsTable::MAX, "sum_partials_many: %d entries", tab.n);
  hipLaunchKernelGGL(sum_partials_many_kernel, dim3((unsigned)tab.block_begin[tab.n]), dim3(256), 0, s, tab);
  MAE_LAUNCH_CHECK();
  return 0;
}

int launch_sum_partials(const float* partial, int G, int C, float* out0, float* out1, int split, hipStream_t s) {
  MAE_REQUIRE(partial && out0 && G > 0 && C > 0 && C % 4 == 0 && (split >= C || out1), "sum_partials: bad arguments (C %% 4 == 0)");
  hipLaunchKernelGGL(sum_partials_kernel, dim3((unsigned)cdiv(C, 32)), dim3(256), 0, s, partial, G, C, out0, out1, split);
  MAE_LAUNCH_CHECK();
  return 0;
}

// The row walk of the two split kernels of this file (layout, fold and launcher tail: kernels.h).  U rows per thread and trip are
// in flight (512 blocks x one 16-byte load per thread ran at 2.6 TB/s).  A row r < rows has the key key(r); a row past the end
// has key -1 and reads as zeros.  fate(r, key, v, d0, acc) adds the row to the column sum, or stores it wherever it goes, or both;
// u ascending inside a trip = r ascending, which fixes the order of the additions.
template <int U, class Key, class Fate>
__device__ __forceinline__ void split_walk(const float* __restrict__ dx, int64_t rows, int D, float* __restrict__ partial, Key key, Fate fate) {
  split_block(D, partial, [&](int RPI, int ro, int d0, f32x4& acc) {
    const int64_t stride = (int64_t)gridDim.x * RPI;
    for (int64_t r0 = (int64_t)blockIdx.x * RPI + ro; r0 < rows; r0 += U * stride) {
      f32x4 v[U];
      int j[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t r = r0 + u * stride;
        const bool live = r < rows;
        v[u] = live ? load4(dx + r * D + d0) : f32x4{0.f, 0.f, 0.f, 0.f};
        j[u] = live ? key(r) : -1;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) fate(r0 + u * stride, j[u], v[u], d0, acc);
    }
  });
}

// dtok = dx with the class-token rows (tok == 0) zeroed; partial = column sums of those rows
template <class T>
__global__ void __launch_bounds__(256) visible_grad_split_kernel(const float* __restrict__ dx,
                                                                 const int32_t* __restrict__ tok, int64_t rows, int D,
                                                                 T* __restrict__ dtok, float* __restrict__ partial) {
  split_walk<4>(dx, rows, D, partial, [&](int64_t r) { return tok[r]; }, [&](int64_t r, int t, f32x4 v, int d0, f32x4& acc) {
    if (t == 0) acc += v;
    if (r < rows) store4(dtok + r * D + d0, t == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : v);
  });
}

int launch_visible_grad_split(const float* dx, const int32_t* tok, int64_t rows, int D, int dt, void* dtok, float* dcls,
                              float* partial, hipStream_t s) {
  MAE_REQUIRE(dx && tok && dtok && dcls && partial && rows > 0 && D % 4 == 0 && D <= 1024,
              "visible_grad_split: bad arguments (need D %% 4 == 0, D <= 1024)");
  return launch_split(rows, D, dt, partial, dcls, s, [&](auto t, dim3 grid, size_t lds) {
    using T = decltype(t);
    hipLaunchKernelGGL(visible_grad_split_kernel<T>, grid, dim3(256), lds, s, dx, tok, rows, D, (T*)dtok, partial);
  });
}

// ---------------------------------------------------------------------------------------------------
// decoder input assembly and its adjoint
// ---------------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(256) decoder_assemble_kernel(const T* __restrict__ xdec,
                                                               const int32_t* __restrict__ inv,
                                                               const float* __restrict__ mask_token,
                                                               const float* __restrict__ pos, int64_t rows, int k, int L,
                                                               int D4, float* __restrict__ out) {
  // D4 threads per row, 256 / D4 rows per block pass: 32-bit index math only (a 64-bit divide per element made this
  // kernel run at half the HBM rate)
  const int rpb = 256 / D4, ro = threadIdx.x / D4, d = (threadIdx.x - ro * D4) * 4;
  if (ro >= rpb) return;
  // four rows per thread and pass: the row's index, then its source row, are two dependent round trips -- with one row in flight per
  // thread the kernel ran at 3.2 TB/s
  constexpr int U = 4;
  const int64_t stride = (int64_t)gridDim.x * rpb;
  for (int64_t r0 = (int64_t)blockIdx.x * rpb + ro; r0 < rows; r0 += U * stride) {
    int j[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { const int64_t r = r0 + u * stride; j[u] = r < rows ? inv[r] : -1; }
    f32x4 v[U], pz[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = r0 + u * stride < rows ? r0 + u * stride : rows - 1;
      const int b = (int)((uint32_t)r / (uint32_t)L);  // rows < 2^31 is checked by the launcher
      const int t = (int)(r - (int64_t)b * L);
      v[u] = (j[u] >= 0) ? load4(xdec + ((int64_t)b * k + j[u]) * (D4 * 4) + d) : load4(mask_token + d);
      pz[u] = load4(pos + t * (D4 * 4) + d);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = r0 + u * stride;
      if (r < rows) store4(out + r * (D4 * 4) + d, v[u] + pz[u]);   // (ordinary stores: 74.6 us against 77.1 non-temporal)
    }
  }
}

int launch_decoder_assemble(const void* xdec, int dt, const int32_t* inv, const float* mask_token, const float* pos,
                            int B, int k, int L, int Dd, float* out, hipStream_t s) {
  MAE_REQUIRE(xdec && inv && mask_token && pos && out && Dd % 4 == 0, "decoder_assemble: bad arguments");
  const int64_t rows = (int64_t)B * L;
  MAE_REQUIRE(Dd / 4 <= 256 && rows < (1ll << 31), "decoder_assemble: Dd <= 1024 and B * L < 2^31");
  const int grid = (int)std::min<int64_t>(cdiv(rows, 256 / (Dd / 4)), 256 * 16);
  with_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(decoder_assemble_kernel<T>, dim3(grid), dim3(256), 0, s, (const T*)xdec, inv, mask_token, pos, rows, k, L, Dd / 4, out);
  });
  MAE_LAUNCH_CHECK();
  return 0;
}

// d_xdec[b*k + inv[r]] = dx[r] for the visible rows; partial = column sums of the masked rows (inv[r] < 0), rows past the end
// joining them as zeros
template <class T>
__global__ void __launch_bounds__(256) decoder_assemble_bwd_kernel(const float* __restrict__ dx,
                                                                   const int32_t* __restrict__ inv, int64_t rows, int k,
                                                                   int L, int D, T* __restrict__ d_xdec,
                                                                   float* __restrict__ partial) {
  split_walk<4>(dx, rows, D, partial, [&](int64_t r) { return inv[r]; }, [&](int64_t r, int j, f32x4 v, int d0, f32x4& acc) {
    if (j < 0) {
      acc += v;
    } else {
      const int64_t b = (uint32_t)r / (uint32_t)L;  // rows < 2^31 (checked by the launcher)
      store4(d_xdec + (b * k + j) * (int64_t)D + d0, v);
    }
  });
}

int launch_decoder_assemble_bwd(const float* dx, const int32_t* inv, int B, int k, int L, int Dd, int dt, void* d_xdec,
                                float* d_mask_token, float* partial, hipStream_t s) {
  MAE_REQUIRE(dx && inv && d_xdec && d_mask_token && partial && Dd % 4 == 0 && Dd <= 1024,
              "decoder_assemble_bwd: bad arguments (need Dd %% 4 == 0, Dd <= 1024)");
  const int64_t rows = (int64_t)B * L;
  MAE_REQUIRE(rows < (1ll << 31), "decoder_assemble_bwd: B * L < 2^31");
  return launch_split(rows, Dd, dt, partial, d_mask_token, s, [&](auto t, dim3 grid, size_t lds) {
    using T = decltype(t);
    hipLaunchKernelGGL(decoder_assemble_bwd_kernel<T>, grid, dim3(256), lds, s, dx, inv, rows, k, L, Dd, (T*)d_xdec, partial);
  });
}

template <class S, class D_>
__global__ void __launch_bounds__(256) cast_kernel(const S* __restrict__ src, D_* __restrict__ dst, int64_t n) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = from_f<D_>(to_f(src[i]));
}

int launch_cast(const void* src, int src_dt, void* dst, int dst_dt, int64_t n, hipStream_t s) {
  MAE_REQUIRE(src && dst && n > 0, "cast: bad arguments");
  MAE_REQUIRE((src_dt == MAE_F32 || src_dt == MAE_BF16) && (dst_dt == MAE_F32 || dst_dt == MAE_BF16),
              "cast: dtypes must be MAE_F32 or MAE_BF16 (got %d -> %d)", src_dt, dst_dt);
  const int grid = (int)std::min<int64_t>(cdiv(n, 256), 256 * 16);
  with_dtype(src_dt, [&](auto a) {
    with_dtype(dst_dt, [&](auto b) {
      using S = decltype(a);
      using D_ = decltype(b);
      hipLaunchKernelGGL((cast_kernel<S, D_>), dim3(grid), dim3(256), 0, s, (const S*)src, (D_*)dst, n);
    });
  });
  MAE_LAUNCH_CHECK();
  return 0;
}

// out[r] = x[r] + pos[r mod L]  (fp32, D/4 float4 per row): the `x + decoder_pos_embed` of decoder.decode()
__global__ void add_rows_pos_kernel(const float* __restrict__ x, const float* __restrict__ pos, int64_t rows, int L, int D4,
                                    float* __restrict__ out) {
  const int64_t n = rows * D4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / D4;
    const int c = (int)(i - r * D4);
    store4(out + i * 4, load4(x + i * 4) + load4(pos + ((r % L) * D4 + c) * 4));
  }
}
int launch_add_rows_pos(const float* x, const float* pos, int64_t rows, int L, int D, float* out, hipStream_t s) {
  MAE_REQUIRE(x && pos && out && rows > 0 && L > 0, "add_rows_pos: bad arguments");
  MAE_REQUIRE(D % 4 == 0 && D >= 4, "add_rows_pos: D = %d must be a positive multiple of 4", D);
  const int grid = (int)std::min<int64_t>(cdiv(rows * (D / 4), 256), 256 * 16);
  hipLaunchKernelGGL(add_rows_pos_kernel, dim3(grid), dim3(256), 0, s, x, pos, rows, L, D / 4, out);
  MAE_LAUNCH_CHECK();
  return 0;
}

// dst[i] (dt) += src[i] (fp32): an extra upstream gradient joins the engine's own one at a tensor boundary
template <class T>
__global__ void add_into_kernel(const float* __restrict__ src, T* __restrict__ dst, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = from_f<T>(to_f(dst[i]) + src[i]);
}
int launch_add_into(const float* src, void* dst, int dst_dt, int64_t n, hipStream_t s) {
  MAE_REQUIRE(src && dst && n > 0, "add_into: bad arguments");
  MAE_REQUIRE(dst_dt == MAE_F32 || dst_dt == MAE_BF16, "add_into: dtype must be MAE_F32 or MAE_BF16 (got %d)", dst_dt);
  const int grid = (int)std::min<int64_t>(cdiv(n, 256), 256 * 16);
  with_dtype(dst_dt, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(add_into_kernel<T>, dim3(grid), dim3(256), 0, s, src, (T*)dst, n); });
  MAE_LAUNCH_CHECK();
  return 0;
}

// The row clear.  The backward pass of the decoder starts from a residual gradient that is zero on every row the prediction head
// never saw: the visible rows (inv[row] >= 0, MAE) or the first T - m rows of every sequence (I-JEPA's predictor); the classifier's
// with cls pooling is zero on every row but the class token's.  Only those rows are cleared here (a quarter of the rows at mask
// ratio 0.75); the norm backward then writes the others.  A row is kept when inv[row] < 0, or without inv when row % Tseq lies in
// [lo, hi).
template <class T>
__global__ void __launch_bounds__(256) zero_rows_kernel(const int32_t* __restrict__ inv, int64_t rows, int Tseq, int lo, int hi, int D4,
                                                        float* __restrict__ dres, T* __restrict__ dres_c) {
  const int lanes = D4 <= 64 ? 64 : 128;   // threads per row: one float4 each, two passes at most for D <= 1024
  const int rpb = 256 / lanes, sub = threadIdx.x / lanes, l = threadIdx.x % lanes;
  for (int64_t row = (int64_t)blockIdx.x * rpb + sub; row < rows; row += (int64_t)gridDim.x * rpb) {
    const int t = (int)(row % Tseq);
    if (inv ? inv[row] < 0 : t >= lo && t < hi) continue;
    for (int c = l; c < D4; c += lanes) {
      store4(dres + row * (int64_t)D4 * 4 + c * 4, f32x4{0.f, 0.f, 0.f, 0.f});
      store4(dres_c + row * (int64_t)D4 * 4 + c * 4, f32x4{0.f, 0.f, 0.f, 0.f});
    }
  }
}

static int launch_zero_rows(const int32_t* inv, int64_t rows, int Tseq, int lo, int hi, int D, int act, float* dres, void* dres_c, hipStream_t s) {
  const int rpb = D / 4 <= 64 ? 4 : 2;
  const int grid = (int)std::min<int64_t>(cdiv(rows, rpb), 8192);
  with_dtype(act, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(zero_rows_kernel<T>, dim3(grid), dim3(256), 0, s, inv, rows, Tseq, lo, hi, D / 4, dres, (T*)dres_c);
  });
  MAE_LAUNCH_CHECK();
  return 0;
}

int launch_zero_unpredicted_rows(const int32_t* inv, int64_t rows, int Tseq, int m, int D, int act, float* dres, void* dres_c, hipStream_t s) {
  MAE_REQUIRE(dres && dres_c && rows > 0 && D % 4 == 0 && Tseq > 0 && m >= 0 && m <= Tseq, "zero_unpredicted_rows: bad arguments");
  return launch_zero_rows(inv, rows, Tseq, Tseq - m, Tseq, D, act, dres, dres_c, s);
}

// cls pooling: every row of dres / dres_c except the class-token row of each image is zero before the blocks' backward
int launch_zero_token_rows(int64_t rows, int L, int D, int act, float* dres, void* dres_c, hipStream_t s) {
  MAE_REQUIRE(dres && dres_c && rows > 0 && L > 0, "zero_token_rows: bad arguments");
  MAE_REQUIRE(D % 4 == 0 && D >= 4 && D <= 1024, "zero_token_rows: D = %d must be a multiple of 4 in [4, 1024]", D);
  MAE_REQUIRE(act == MAE_F32 || act == MAE_BF16, "zero_token_rows: dtype must be MAE_F32 or MAE_BF16 (got %d)", act);
  return launch_zero_rows(nullptr, rows, L, 0, 1, D, act, dres, dres_c, s);
}

}  // namespace mae

extern "C" int mae_assemble_visible(float* x, const int32_t* tok32, const float* cls, const float* pos, int64_t rows, int32_t dim, void* stream) {
  return mae::launch_assemble_visible(x, tok32, cls, pos, rows, dim, (hipStream_t)stream);
}

extern "C" int mae_visible_grad_split(const float* dx, const int32_t* tok32, int64_t rows, int32_t dim, int32_t dtype, void* dtok, float* dcls,
                                      float* partial, void* stream) {
  return mae::launch_visible_grad_split(dx, tok32, rows, dim, dtype, dtok, dcls, partial, (hipStream_t)stream);
}

extern "C" int mae_decoder_assemble(const void* xdec, int32_t dtype, const int32_t* inv, const float* mask_token, const float* pos, int32_t batch,
                                    int32_t num_keep, int32_t seq_len, int32_t dim, float* out, void* stream) {
  MAE_REQUIRE(batch > 0 && num_keep > 0 && num_keep <= seq_len, "mae_decoder_assemble: bad arguments");
  return mae::launch_decoder_assemble(xdec, dtype, inv, mask_token, pos, batch, num_keep, seq_len, dim, out, (hipStream_t)stream);
}

extern "C" int mae_decoder_assemble_bwd(const float* dx, const int32_t* inv, int32_t batch, int32_t num_keep, int32_t seq_len, int32_t dim,
                                        int32_t dtype, void* d_xdec, float* d_mask_token, float* partial, void* stream) {
  MAE_REQUIRE(batch > 0 && num_keep > 0 && num_keep <= seq_len, "mae_decoder_assemble_bwd: bad arguments");
  return mae::launch_decoder_assemble_bwd(dx, inv, batch, num_keep, seq_len, dim, dtype, d_xdec, d_mask_token, partial, (hipStream_t)stream);
}

extern "C" int mae_zero_unpredicted_rows(const int32_t* inv, int64_t rows, int32_t seq_len, int32_t num_pred, int32_t dim, int32_t dtype,
                                         float* dres, void* dres_c, void* stream) {
  return mae::launch_zero_unpredicted_rows(inv, rows, seq_len, num_pred, dim, dtype, dres, dres_c, (hipStream_t)stream);
}

extern "C" int mae_zero_token_rows(int64_t rows, int32_t seq_len, int32_t dim, int32_t dtype, float* dres, void* dres_c, void* stream) {
  return mae::launch_zero_token_rows(rows, seq_len, dim, dtype, dres, dres_c, (hipStream_t)stream);
}

// single-kernel entries (parity tests): the engine-only element kernels of this file, see mae_hip.h
extern "C" int mae_cast(const void* src, int32_t src_dtype, void* dst, int32_t dst_dtype, int64_t n, void* stream) {
  return mae::launch_cast(src, src_dtype, dst, dst_dtype, n, (hipStream_t)stream);
}

extern "C" int mae_add_rows_pos(const float* x, const float* pos, int64_t rows, int32_t seq_len, int32_t dim, float* out, void* stream) {
  return mae::launch_add_rows_pos(x, pos, rows, seq_len, dim, out, (hipStream_t)stream);
}

extern "C" int mae_add_into(const float* src, void* dst, int32_t dst_dtype, int64_t n, void* stream) {
  return mae::launch_add_into(src, dst, dst_dtype, n, (hipStream_t)stream);
}
