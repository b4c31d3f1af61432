// fc_sign_gram.hip — the clients' geometry straight from scaled-sign packets for MI355X (gfx950):
// the M x M Gram matrix and the products with a dense vector, without one decoded row.
//
// A sign packet decodes to d_i[t] = b_i[t] ? -s_i : +s_i, so
//   <d_i, d_j> = s_i s_j (n - 2 H_ij),   H_ij = popcount(words_i XOR words_j)   (bits at and past n
//                                         and the pad words are zero in every packet)
//   <d_i, v>   = s_i D_i,                D_i  = sum_t (b_i[t] ? -(double)v[t] : +(double)v[t])
// The Gram matrix of a round is a Hamming-distance matrix over M bit strings: integer counting,
// free of any order of summation, and one IEEE float64 multiply per entry at the very end.
//
// Both kernels stage a span of W consecutive words of every client in LDS TRANSPOSED, img[w][row]
// with a row stride of S = 8 ceil(m / 8) + 4 words: a thread then reads the words of eight
// consecutive clients at one word position as two 16-B LDS reads, and lanes that differ in the
// client read consecutive banks.  A span comes in with coalesced 16-B global loads (a wave: 8 rows
// x 128 bytes) and goes to LDS as four 4-B stores per lane (2-way bank conflicts at most, which a
// 4-B store hides); rows m .. S - 5 and words at and past fc_sign_words(n) are staged as zero, so
// the inner loops have no bounds branch.
//
// k_sign_gram, workgroup = a slice of spans that depends on n and m alone.  The upper triangle of
//   the pair matrix is cut into T = t (t + 1) / 2 tiles of 8 x 8 pairs (t = ceil(m / 8)); thread
//   (k, tile) owns one tile at the word positions w = k, k + ks, ... of every span (ks = min(16,
//   1024 / T): 952 of 960 launched threads work at m = 128), holding the 64 counts in registers for
//   the whole slice: per word 2 + 2 LDS reads and 64 x (v_xor_b32, v_bcnt_u32_b32 accumulating).
//   The next span's global loads are in flight while a span is counted.  After the slice the ks
//   threads of a tile add their counts in LDS (integer atomics: any order, the same integers) and
//   the workgroup stores its uint32 count matrix to ITS part of the workspace.
// k_sign_gram_fin adds the parts (integers), forms fl64(s_i) fl64(s_j) (exact: 48 significant
//   bits) times (double)(n - 2 H) (exact: below 2^32 in magnitude), writes both triangles, and NaN
//   into the rows and columns of a client whose scale is not finite.
//
// k_sign_dot, workgroup = a slice of 64-word spans: thread (k, i) owns client i at the word
//   positions w = k, k + ks, ... (ks the largest power of two with m ks <= 1024, 64 at most); per
//   word it reads its word and v's 32 floats from LDS (eight 16-B reads, the same address in every
//   lane of a phase: a broadcast), flips each float's sign by its bit and adds it as a double into
//   one of four accumulators (element b into b % 4), which it keeps for the whole slice: no
//   cross-lane reduction.  With v == NULL it counts set bits instead.  The sum of v's squares is
//   taken while v is staged.  Partials go to the workspace; k_sign_dot_fin (one workgroup per
//   output) adds them in a fixed order (strided per thread, a butterfly per wave, the waves in order), multiplies by fl64(s_i) and writes NaN for a
//   non-finite s_i or, all outputs, for a non-finite v.
// No floating-point atomics, no workgroup waits for another, and every workspace word that is read
// was written by the same call (no zeroing).
#include "fc_state.h"
#include "fc_sign_host.h"

namespace fc {

constexpr int kSGMaxBlock = 1024;
constexpr int kSGMaxSplit = 16;                   // word phases per tile at most
constexpr int kSGSteps = 8;                       // words per phase and span: W = kSGSteps * ks
constexpr int kSGLoads = 4;                       // 16-B loads per thread and span at most
constexpr uint32_t kSGSlices = 512;               // workgroups (parts of the workspace) at most
constexpr int kSGFinGroups = 16;                  // k_sign_gram_fin: slice groups per workgroup
constexpr int kSDWords = 64;                      // k_sign_dot: words per span
constexpr int kSDVStride = 36;                    // floats per staged word of v (32 + 4: banks)
constexpr uint32_t kSDSlices = 512;
constexpr int kSDStride = 1024;                   // partials per slice of the workspace
constexpr int kSDFinBlock = 1024;                 // k_sign_dot_fin: threads per output

struct SGramArgs {
  const fc_packet_view* views;                    // DEVICE array of m views
  uint32_t* part;                                 // [slices][64][T] partial counts
  double* gram;                                   // [m][m]
  uint64_t n, n_words;
  uint32_t m, t, T, S, ks, W, chunks;             // chunks: 16-B chunks of a span, pad rows included
  uint32_t nspans, sps, slices;                   // spans; spans per slice; slices launched
};

// Tile r of the upper triangle in row-major order: (ti, tj), ti <= tj < t.
__device__ __forceinline__ void sgram_tile(uint32_t r, uint32_t t, uint32_t* ti, uint32_t* tj) {
  uint32_t i = 0;
  while (r >= t - i) { r -= t - i; ++i; }
  *ti = i; *tj = i + r;
}

__device__ __forceinline__ bool sign_scale_bad(float s) {
  return (__float_as_uint(s) & 0x7f800000u) == 0x7f800000u;
}

// 16-B chunk c of the span that starts at word w0: its row, its first word inside the span, and
// the four words (zero for a pad row and at or past n_words, a multiple of 4).  Lane l of a wave:
// row l % 8 of a group of eight rows, chunk l / 8 of eight consecutive ones.
__device__ __forceinline__ void sign_span_place(uint32_t c, uint32_t q_per_row, uint32_t* row,
                                                uint32_t* word) {
  const uint32_t g = c >> 3, rg = g / q_per_row;
  *row = rg * 8 + (c & 7u);
  *word = 4 * (g - rg * q_per_row);
}

__device__ __forceinline__ fc_u32x4 sign_span_load(const uint64_t* s_words, uint32_t c, uint32_t q_per_row,
                                                   uint32_t m, uint64_t w0, uint64_t n_words,
                                                   uint32_t* row, uint32_t* word) {
  sign_span_place(c, q_per_row, row, word);
  const uint64_t w = w0 + *word;
  fc_u32x4 x = {0u, 0u, 0u, 0u};
  if (*row < m && w < n_words) x = *(const FC_G fc_u32x4*)((const FC_G uint32_t*)s_words[*row] + w);
  return x;
}

__device__ __forceinline__ void sign_span_store(uint32_t* img, uint32_t S, uint32_t row, uint32_t word,
                                                fc_u32x4 x) {
  uint32_t* p = img + (size_t)word * S + row;
  p[0] = x.x; p[S] = x.y; p[2 * S] = x.z; p[3 * S] = x.w;
}

__global__ __launch_bounds__(kSGMaxBlock) void k_sign_gram(SGramArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sg_lds[];
  uint32_t* img = reinterpret_cast<uint32_t*>(sg_lds);      // [W][S]; after the slice [64][T]
  __shared__ uint64_t s_words[kGMaxM];
  const uint32_t tid = threadIdx.x, nthr = blockDim.x;
  const uint32_t S = a.S, T = a.T, ks = a.ks, Q = a.W / 4;
  if (tid < a.m) s_words[tid] = (uint64_t)((const FC_G fc_packet_view*)a.views + tid)->bitmap;
  const bool worker = tid < T * ks;
  const uint32_t k = worker ? tid / T : 0u, tile = worker ? tid - k * T : 0u;
  uint32_t ti, tj;
  sgram_tile(tile, a.t, &ti, &tj);
  uint32_t acc[64];
#pragma unroll
  for (int e = 0; e < 64; ++e) acc[e] = 0u;
  const uint32_t sp0 = blockIdx.x * a.sps, sp1 = min(sp0 + a.sps, a.nspans);
  __syncthreads();

  fc_u32x4 pre[kSGLoads];
  auto fetch = [&](uint32_t sp) {
#pragma unroll
    for (int j = 0; j < kSGLoads; ++j) {
      const uint32_t c = tid + (uint32_t)j * nthr;
      uint32_t row, word;
      pre[j] = fc_u32x4{0u, 0u, 0u, 0u};
      if (c < a.chunks)
        pre[j] = sign_span_load(s_words, c, Q, a.m, (uint64_t)sp * a.W, a.n_words, &row, &word);
    }
  };
  fetch(sp0);
  for (uint32_t sp = sp0; sp < sp1; ++sp) {
    __syncthreads();                               // the previous span is counted
#pragma unroll
    for (int j = 0; j < kSGLoads; ++j) {
      const uint32_t c = tid + (uint32_t)j * nthr;
      if (c < a.chunks) {
        uint32_t row, word;
        sign_span_place(c, Q, &row, &word);
        sign_span_store(img, S, row, word, pre[j]);
      }
    }
    __syncthreads();
    if (sp + 1 < sp1) fetch(sp + 1);               // in flight while this span is counted
    if (worker) {
      const uint32_t* pa = img + (size_t)k * S + 8 * ti;
      const uint32_t* pb = img + (size_t)k * S + 8 * tj;
#pragma unroll 1
      for (int s = 0; s < kSGSteps; ++s) {
        const fc_u32x4 a0 = *reinterpret_cast<const fc_u32x4*>(pa);
        const fc_u32x4 a1 = *reinterpret_cast<const fc_u32x4*>(pa + 4);
        const fc_u32x4 b0 = *reinterpret_cast<const fc_u32x4*>(pb);
        const fc_u32x4 b1 = *reinterpret_cast<const fc_u32x4*>(pb + 4);
        const uint32_t A[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const uint32_t B[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int x = 0; x < 8; ++x)
#pragma unroll
          for (int y = 0; y < 8; ++y) acc[x * 8 + y] += (uint32_t)__popc(A[x] ^ B[y]);
        pa += (size_t)ks * S;
        pb += (size_t)ks * S;
      }
    }
  }
  // ---- the ks phases of a tile added in LDS, [entry][tile]; then this workgroup's part ----
  __syncthreads();
  const uint32_t E = 64 * T;
  for (uint32_t i = tid; i < E; i += nthr) img[i] = 0u;
  __syncthreads();
  if (worker) {
#pragma unroll
    for (int e = 0; e < 64; ++e) atomicAdd(&img[(uint32_t)e * T + tile], acc[e]);
  }
  __syncthreads();
  uint32_t* part = a.part + (uint64_t)blockIdx.x * E;
  for (uint32_t i = tid; i < E; i += nthr) part[i] = img[i];
}

// Workgroup = 64 consecutive entries (entry * T + tile) x kSGFinGroups groups of slices.
__global__ __launch_bounds__(64 * kSGFinGroups) void k_sign_gram_fin(SGramArgs a) {
  __shared__ uint32_t s_sum[kSGFinGroups][64];
  const uint32_t xl = threadIdx.x & 63u, g = threadIdx.x >> 6;
  const uint32_t E = 64 * a.T, x = blockIdx.x * 64 + xl;
  uint32_t h = 0;
  if (x < E)
    for (uint32_t sl = g; sl < a.slices; sl += kSGFinGroups) h += a.part[(uint64_t)sl * E + x];
  s_sum[g][xl] = h;
  __syncthreads();
  if (g != 0 || x >= E) return;
  h = 0;
#pragma unroll
  for (int i = 0; i < kSGFinGroups; ++i) h += s_sum[i][xl];
  const uint32_t e = x / a.T, tile = x - e * a.T;
  uint32_t ti, tj;
  sgram_tile(tile, a.t, &ti, &tj);
  const uint32_t i = 8 * ti + (e >> 3), j = 8 * tj + (e & 7u);
  if (i >= a.m || j >= a.m || i > j) return;
  const FC_G fc_packet_view* vw = (const FC_G fc_packet_view*)a.views;
  const float si = (float)((const FC_G fc_packet_hdr*)vw[i].hdr)->p;
  const float sj = (float)((const FC_G fc_packet_hdr*)vw[j].hdr)->p;
  const int64_t d = (int64_t)a.n - 2 * (int64_t)h;
  double v = ((double)si * (double)sj) * (double)d;
  if (sign_scale_bad(si) || sign_scale_bad(sj)) v = __longlong_as_double(0x7ff8000000000000ll);
  a.gram[(uint64_t)i * a.m + j] = v;
  a.gram[(uint64_t)j * a.m + i] = v;
}

struct SDotArgs {
  const fc_packet_view* views;
  const float* v;                                 // DEVICE float32[n], or nullptr: all ones
  double* part;                                   // [slices][kSDStride]: entry k * m + i
  double* qpart;                                  // [slices] partial sums of v's squares
  double* out;                                    // [m + 1]
  uint64_t n, n_words;
  uint32_t m, S, ks, chunks;                      // chunks: 16-B chunks of a span's words
  uint32_t nspans, sps, slices;
};

template <bool DENSE>
__global__ __launch_bounds__(kSGMaxBlock) void k_sign_dot(SDotArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t wimg[kSDWords * (kGMaxM + 4)];   // [w][S]
  __shared__ __attribute__((aligned(16))) float vimg[kSDWords * kSDVStride];
  __shared__ uint64_t s_words[kGMaxM];
  __shared__ double swq[kSGMaxBlock / 64];
  const uint32_t tid = threadIdx.x, nthr = blockDim.x;
  const uint32_t S = a.S, m = a.m, ks = a.ks;
  if (tid < m) s_words[tid] = (uint64_t)((const FC_G fc_packet_view*)a.views + tid)->bitmap;
  const bool worker = tid < m * ks;
  const uint32_t k = worker ? tid / m : 0u, i = worker ? tid - k * m : 0u;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  uint32_t cnt = 0u;
  double q = 0.0;
  const uint32_t sp0 = blockIdx.x * a.sps, sp1 = min(sp0 + a.sps, a.nspans);
  for (uint32_t sp = sp0; sp < sp1; ++sp) {
    const uint64_t w0 = (uint64_t)sp * kSDWords;
    __syncthreads();                               // the previous span is done with (and s_words set)
    for (uint32_t c = tid; c < a.chunks; c += nthr) {
      uint32_t row, word;
      const fc_u32x4 x = sign_span_load(s_words, c, kSDWords / 4, m, w0, a.n_words, &row, &word);
      sign_span_store(wimg, S, row, word, x);
    }
    if (DENSE) {
      // v's 32 floats of each of the span's words; nothing of v is read at or past n
      for (uint32_t c = tid; c < kSDWords * 8; c += nthr) {
        const uint32_t w = c >> 3, j = c & 7u;
        const float4 f = load4_plain(a.v, (w0 + w) * 32 + 4 * j, a.n);
        *reinterpret_cast<float4*>(&vimg[w * kSDVStride + 4 * j]) = f;
        q = fma((double)f.x, (double)f.x, q); q = fma((double)f.y, (double)f.y, q);
        q = fma((double)f.z, (double)f.z, q); q = fma((double)f.w, (double)f.w, q);
      }
    }
    __syncthreads();
    if (!worker) continue;
    for (uint32_t w = k; w < (uint32_t)kSDWords; w += ks) {
      const uint32_t bits = wimg[w * S + i];
      if (!DENSE) {
        cnt += (uint32_t)__popc(bits);
        continue;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float4 f = *reinterpret_cast<const float4*>(&vimg[w * kSDVStride + 4 * j]);
        const float x[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const uint32_t flip = (bits << (31 - (4 * j + b))) & 0x80000000u;
          acc[b] = acc[b] + (double)__uint_as_float(__float_as_uint(x[b]) ^ flip);
        }
      }
    }
  }
  if (worker) {
    const double s = DENSE ? (acc[0] + acc[1]) + (acc[2] + acc[3]) : (double)cnt;
    a.part[(uint64_t)blockIdx.x * kSDStride + tid] = s;       // tid == k * m + i
  }
  if (DENSE) {
    const double s = dot_wave_sum(q);
    if ((tid & 63u) == 0) swq[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
      for (uint32_t w = 0; w < nthr / 64; ++w) t = t + swq[w];
      a.qpart[blockIdx.x] = t;
    }
  }
}

// One workgroup per output: out[i] (i < m) = fl64(s_i) * D_i, D_i the client's partials added
// (thread t: those of flat index t, t + kSDFinBlock, ... over (slice, phase), then the butterfly
// per wave, then the waves in order), or n - 2 popcount_i for the all-ones vector; out[m] = the
// sum of v's squares added the same way, or (double)n.
__global__ __launch_bounds__(kSDFinBlock) void k_sign_dot_fin(SDotArgs a) {
  __shared__ double s_q[kSDFinBlock / 64], s_s[kSDFinBlock / 64];
  const uint32_t i = blockIdx.x, tid = threadIdx.x;
  const bool dense = a.v != nullptr;
  double q = 0.0, s = 0.0;
  if (dense)
    for (uint32_t sl = tid; sl < a.slices; sl += kSDFinBlock) q = q + a.qpart[sl];
  if (i < a.m) {
    const uint32_t total = a.slices * a.ks;
    for (uint32_t e = tid; e < total; e += kSDFinBlock) {
      const uint32_t sl = e / a.ks, k = e - sl * a.ks;
      s = s + a.part[(uint64_t)sl * kSDStride + k * a.m + i];
    }
  }
  q = dot_wave_sum(q);
  s = dot_wave_sum(s);
  if ((tid & 63u) == 0) { s_q[tid >> 6] = q; s_s[tid >> 6] = s; }
  __syncthreads();
  if (tid != 0) return;
  q = 0.0; s = 0.0;
  for (int w = 0; w < kSDFinBlock / 64; ++w) { q = q + s_q[w]; s = s + s_s[w]; }
  if (!dense) q = (double)a.n;
  bool bad = (__double_as_longlong(q) & 0x7ff0000000000000ll) == 0x7ff0000000000000ll;
  if (i < a.m) {
    if (!dense) s = (double)a.n - 2.0 * s;         // exact: integers below 2^33
    const FC_G fc_packet_view* vw = (const FC_G fc_packet_view*)a.views;
    const float sc = (float)((const FC_G fc_packet_hdr*)vw[i].hdr)->p;
    s = (double)sc * s;
    bad |= sign_scale_bad(sc);
  } else {
    s = q;
  }
  if (bad) s = __longlong_as_double(0x7ff8000000000000ll);
  a.out[i] = s;
}

}  // namespace fc

using namespace fc;

// Geometry from n and m alone.
namespace {
struct SGramGeom {
  uint32_t t, T, S, ks, W, chunks, block, nspans, sps, slices;
  uint64_t n_words;
  size_t lds, bytes;
};
SGramGeom sgram_geom(uint64_t n, int m) {
  SGramGeom g;
  g.t = ((uint32_t)m + 7) / 8;
  g.T = g.t * (g.t + 1) / 2;
  g.S = 8 * g.t + 4;
  g.ks = std::min<uint32_t>(kSGMaxSplit, kSGMaxBlock / g.T);
  g.W = kSGSteps * g.ks;
  g.chunks = 8 * g.t * (g.W / 4);
  const uint32_t need = std::max(g.T * g.ks, (g.chunks + kSGLoads - 1) / kSGLoads);
  g.block = (need + 63) / 64 * 64;
  g.n_words = sign_words(n);
  g.nspans = (uint32_t)((g.n_words + g.W - 1) / g.W);
  const uint32_t cap = std::min<uint32_t>(g.nspans, kSGSlices);
  g.sps = (g.nspans + cap - 1) / cap;
  g.slices = (g.nspans + g.sps - 1) / g.sps;                         // <= cap
  g.lds = std::max((size_t)g.W * g.S, (size_t)64 * g.T) * sizeof(uint32_t);
  g.bytes = ((size_t)cap * 64 * g.T * sizeof(uint32_t) + 255) & ~(size_t)255;
  return g;
}
struct SDotGeom {
  uint32_t S, ks, chunks, block, nspans, sps, slices;
  uint64_t n_words;
  size_t part_bytes, bytes;
};
SDotGeom sdot_geom(uint64_t n, int m) {
  SDotGeom g;
  const uint32_t rows = ((uint32_t)m + 7) / 8 * 8;
  g.S = rows + 4;
  g.ks = 1;
  while (g.ks < (uint32_t)kSDWords && 2 * g.ks * (uint32_t)m <= (uint32_t)kSGMaxBlock) g.ks *= 2;
  g.chunks = rows * (kSDWords / 4);
  g.block = ((uint32_t)m * g.ks + 63) / 64 * 64;
  g.n_words = sign_words(n);
  g.nspans = (uint32_t)((g.n_words + kSDWords - 1) / kSDWords);
  const uint32_t cap = std::min<uint32_t>(g.nspans, kSDSlices);
  g.sps = (g.nspans + cap - 1) / cap;
  g.slices = (g.nspans + g.sps - 1) / g.sps;                         // <= cap
  g.part_bytes = (size_t)cap * kSDStride * sizeof(double);
  g.bytes = g.part_bytes + (((size_t)cap * sizeof(double) + 255) & ~(size_t)255);
  return g;
}
}  // namespace

extern "C" {

size_t fc_sign_gram_workspace_bytes(uint64_t n, int m) {
  if (n == 0 || n > 0xffffffffull || m < 1 || m > FC_GRAM_MAX_M) return 0;
  return sgram_geom(n, m).bytes;
}

int fc_sign_gram(const fc_packet_view* views_dev, int m, uint64_t n, double* gram, void* ws,
                 size_t ws_bytes, fc_stream_t stream) {
  FC_CHECK(views_dev != nullptr, "views_dev is NULL");
  FC_CHECK(gram != nullptr, "gram is NULL");
  FC_CHECK(ws != nullptr, "workspace is NULL");
  FC_CHECK(m >= 1 && m <= FC_GRAM_MAX_M, "m=%d outside [1, %d]", m, FC_GRAM_MAX_M);
  FC_CHECK(n >= 1 && n <= 0xffffffffull, "n=%llu outside [1, 2^32-1]", (unsigned long long)n);
  FC_CHECK(((uintptr_t)gram & 15) == 0, "gram must be 16-byte aligned");
  FC_CHECK(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
  const SGramGeom g = sgram_geom(n, m);
  if (ws_bytes < g.bytes)
    return fail(FC_ERR_WORKSPACE, "workspace %zu B < %zu B needed", ws_bytes, g.bytes);
  SGramArgs a;
  memset(&a, 0, sizeof a);
  a.views = views_dev; a.part = reinterpret_cast<uint32_t*>(ws); a.gram = gram;
  a.n = n; a.n_words = g.n_words; a.m = (uint32_t)m; a.t = g.t; a.T = g.T; a.S = g.S; a.ks = g.ks;
  a.W = g.W; a.chunks = g.chunks; a.nspans = g.nspans; a.sps = g.sps; a.slices = g.slices;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sign_gram, dim3(g.slices), dim3(g.block), g.lds, s, a);
  FC_LAUNCHED("k_sign_gram");
  hipLaunchKernelGGL(k_sign_gram_fin, dim3(g.T), dim3(64 * kSGFinGroups), 0, s, a);
  FC_LAUNCHED("k_sign_gram_fin");
  return FC_OK;
}

size_t fc_sign_dot_workspace_bytes(uint64_t n, int m) {
  if (n == 0 || n > 0xffffffffull || m < 1 || m > FC_GRAM_MAX_M) return 0;
  return sdot_geom(n, m).bytes;
}

int fc_sign_dot(const fc_packet_view* views_dev, int m, uint64_t n, const float* v, double* out,
                void* ws, size_t ws_bytes, fc_stream_t stream) {
  FC_CHECK(views_dev != nullptr, "views_dev is NULL");
  FC_CHECK(out != nullptr, "out is NULL");
  FC_CHECK(ws != nullptr, "workspace is NULL");
  FC_CHECK(m >= 1 && m <= FC_GRAM_MAX_M, "m=%d outside [1, %d]", m, FC_GRAM_MAX_M);
  FC_CHECK(n >= 1 && n <= 0xffffffffull, "n=%llu outside [1, 2^32-1]", (unsigned long long)n);
  FC_CHECK(((uintptr_t)v & 15) == 0, "v must be 16-byte aligned");
  FC_CHECK(((uintptr_t)out & 15) == 0, "out must be 16-byte aligned");
  FC_CHECK(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
  const SDotGeom g = sdot_geom(n, m);
  if (ws_bytes < g.bytes)
    return fail(FC_ERR_WORKSPACE, "workspace %zu B < %zu B needed", ws_bytes, g.bytes);
  SDotArgs a;
  memset(&a, 0, sizeof a);
  a.views = views_dev; a.v = v; a.out = out; a.n = n; a.n_words = g.n_words; a.m = (uint32_t)m;
  a.part = reinterpret_cast<double*>(ws);
  a.qpart = reinterpret_cast<double*>(static_cast<char*>(ws) + g.part_bytes);
  a.S = g.S; a.ks = g.ks; a.chunks = g.chunks; a.nspans = g.nspans; a.sps = g.sps; a.slices = g.slices;
  hipStream_t s = (hipStream_t)stream;
  if (v) hipLaunchKernelGGL(k_sign_dot<true>, dim3(g.slices), dim3(g.block), 0, s, a);
  else hipLaunchKernelGGL(k_sign_dot<false>, dim3(g.slices), dim3(g.block), 0, s, a);
  FC_LAUNCHED("k_sign_dot");
  hipLaunchKernelGGL(k_sign_dot_fin, dim3((uint32_t)m + 1), dim3(kSDFinBlock), 0, s, a);
  FC_LAUNCHED("k_sign_dot_fin");
  return FC_OK;
}

}  // extern "C"
