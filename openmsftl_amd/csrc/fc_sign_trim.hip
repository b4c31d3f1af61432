// fc_sign_trim.hip — coordinate-wise trimmed mean (and median) of a round's scaled-sign packets
// for MI355X (gfx950): fc_packets_trim's definition on the columns d_i[t] = b_i[t] ? -s_i : +s_i,
// without one decoded row and without sorting anything per coordinate.
//
// A column holds only the values -|s_i| and +|s_i| (a client whose scale carries a sign bit is the
// client with |s_i| and every bit flipped; a NaN scale gives a NaN whatever the bit), so np.sort's
// order of a column follows from the order of the m scales alone:
//   the negatives first, by DESCENDING |s_i|;  the positives after them, by ASCENDING |s_i|
//   (+inf last of them);  every NaN after that.
// -0.0 and +0.0 of a zero scale meet in the middle, where np.sort holds them equal, and tied
// scales give equal values: the sum cannot tell their order.
//
// k_sign_trim, one launch, the grid a function of n alone.
//   Ranking, once per workgroup: thread i < m reads client i's scale from its header and makes the
//   key |s_i|'s bits (monotone in |s_i| for every non-NaN float, +inf the largest) or 0xffffffff
//   for a NaN; its rank is the count of keys below its own, ties broken by the client index
//   (m^2 <= 16 K LDS reads per workgroup, all broadcasts).  The clients go to LDS in rank order as
//   16-byte entries {word pointer, |s_i| (the NaN itself), flip mask}; the host reads no header.
//   The walk, lane = one uint32 word = 32 consecutive coordinates (k_sign_reduce_lane's layout: a
//   client's words reach a wave as one coalesced 256-B load, no bit crosses a lane, kSTDepth
//   clients' words are requested before the first is used).  Per coordinate a float32 accumulator
//   from +0.0 and a position counter that starts at -b:
//     pass 1, the non-NaN ranks descending: a set bit takes -|s|;
//     pass 2, all ranks ascending: a clear bit takes +|s|; a NaN client is taken whatever its bit.
//   A taken value is added (__fadd_rn) when the counter is below m - 2b (unsigned: inside the rank
//   window [b, m - b)), and the counter moves on.  What is outside the window adds +0.0 instead,
//   which cannot change an accumulator that started at +0.0 (it never holds -0.0: x + -x and
//   +0.0 + -0.0 round to +0.0).  One __fdiv_rn by float32(m - 2b), eight 16-B stores per lane.
//   A step costs six vector instructions per coordinate.  The steps that cannot land in the window
//   are cheaper: the first b of pass 1 stand at positions below b and only move the counter (two
//   instructions), the last b of pass 2 stand at positions >= m - b and are not walked.  So
//   2 m - 2 b full steps, b counting steps; the words are read (2 m - b) N / 8 bytes.
// No workspace, no floating-point atomics, no workgroup waits for another.
#include "fc_state.h"
#include "fc_sign_host.h"

namespace fc {

constexpr int kSTDepth = 4;                       // clients' words requested before the first is used

struct STrimArgs {
  const fc_packet_view* views;                    // DEVICE array of m views
  float* out;                                     // [n]
  uint64_t n, n_words;
  uint32_t m, trim, span;                         // span = m - 2 trim
  float div;                                      // float32(span)
};
struct STrimClient {                              // 16 bytes in LDS: one ds_read_b128
  uint64_t words;                                 // the client's word pointer
  float s;                                        // |s_i|; a NaN scale as it is
  uint32_t flip;                                  // all ones for a non-NaN scale with the sign bit set
};

// One IEEE float32 add (v_add_f32, round to nearest even: __fadd_rn's instruction) that the
// compiler cannot pair.  Written as __fadd_rn, the 32 adds of a step are SLP-packed two by two
// into v_pk_add_f32, whose operands must sit in register pairs: the kernel then needs 110 VGPRs
// (4 waves per SIMD) instead of 80 (6) and measured 1.28x (128 x 16 M) and 1.35x (32 x 128 M) the
// time.  A plain VOP2 instruction: no wait states of its own, and not volatile, so it is scheduled
// like any other add.
__device__ __forceinline__ float add_f32_unpacked(float x, float y) {
  float r;
  asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
  return r;
}

__global__ __launch_bounds__(kBlock) void k_sign_trim(STrimArgs a) {
  __shared__ STrimClient s_cl[kGMaxM];            // by rank
  __shared__ uint32_t s_key[kGMaxM];
  __shared__ uint32_t s_nn;                       // clients whose scale is no NaN: ranks [0, s_nn)
  const uint32_t tid = threadIdx.x, m = a.m;
  uint32_t key = 0u, sbits = 0u;
  uint64_t wptr = 0ull;
  if (tid < m) {
    const FC_G fc_packet_view* v = (const FC_G fc_packet_view*)a.views + tid;
    wptr = (uint64_t)v->bitmap;
    sbits = __float_as_uint((float)((const FC_G fc_packet_hdr*)v->hdr)->p);
    key = (sbits & 0x7fffffffu) > 0x7f800000u ? 0xffffffffu : sbits & 0x7fffffffu;
    s_key[tid] = key;
  }
  __syncthreads();
  if (tid < m) {
    uint32_t rank = 0u, nn = 0u;
    for (uint32_t j = 0; j < m; ++j) {
      const uint32_t kj = s_key[j];
      rank += (kj < key) | ((kj == key) & (j < tid));
      nn += kj != 0xffffffffu;
    }
    const bool nan = key == 0xffffffffu;
    STrimClient c;
    c.words = wptr;
    c.s = __uint_as_float(nan ? sbits : key);
    c.flip = !nan && (sbits >> 31) ? 0xffffffffu : 0u;
    s_cl[rank] = c;                               // rank < m: a permutation of [0, m)
    if (tid == 0) s_nn = nn;
  }
  __syncthreads();
  const uint64_t wi = (uint64_t)blockIdx.x * kBlock + tid;            // this lane's word
  const uint64_t c0 = 32 * wi;                                       // its first coordinate
  if (!(wi < a.n_words && c0 < a.n)) return;
  const uint32_t nn = s_nn, span = a.span;
  float acc[32];
  uint32_t cnt[32];
#pragma unroll
  for (int b = 0; b < 32; ++b) { acc[b] = 0.f; cnt[b] = 0u - a.trim; }
  // take: the bits whose client gives v to its column now
  auto step = [&](uint32_t take, float v) {
#pragma unroll
    for (int b = 0; b < 32; ++b) {
      const uint32_t mk = (uint32_t)((int32_t)(take << (31 - b)) >> 31);      // bit b everywhere
      const float x = cnt[b] < span ? v : 0.f;
      acc[b] = add_f32_unpacked(acc[b], __uint_as_float(__float_as_uint(x) & mk));
      cnt[b] -= mk;
    }
  };
  // a step that cannot land in the window: the counters alone move on
  auto count = [&](uint32_t take) {
#pragma unroll
    for (int b = 0; b < 32; ++b) cnt[b] += (take >> b) & 1u;
  };
  // ---- pass 1: the negatives, most negative first.  Step j stands at a position <= j, so the
  // first b steps lie below the window whatever their bits are: a loop of their own ----
  const uint32_t lo = nn - min(nn, a.trim);                           // ranks [lo, nn) only count
  for (uint32_t r0 = nn; r0 > lo; r0 -= min(r0 - lo, (uint32_t)kSTDepth)) {
    uint32_t w[kSTDepth];
#pragma unroll
    for (int d = 0; d < kSTDepth; ++d) {
      w[d] = 0u;                                                      // (counts nothing)
      if ((uint32_t)d < r0 - lo) {
        const STrimClient c = s_cl[r0 - 1u - (uint32_t)d];
        w[d] = ((const FC_G uint32_t*)c.words)[wi] ^ c.flip;
      }
    }
#pragma unroll
    for (int d = 0; d < kSTDepth; ++d) count(w[d]);
  }
  for (uint32_t r0 = lo; r0 > 0u; r0 -= min(r0, (uint32_t)kSTDepth)) {
    uint32_t w[kSTDepth];
    float s[kSTDepth];
#pragma unroll
    for (int d = 0; d < kSTDepth; ++d) {
      w[d] = 0u; s[d] = 0.f;
      if ((uint32_t)d < r0) {
        const STrimClient c = s_cl[r0 - 1u - (uint32_t)d];
        w[d] = ((const FC_G uint32_t*)c.words)[wi] ^ c.flip;
        s[d] = c.s;
      }
    }
#pragma unroll
    for (int d = 0; d < kSTDepth; ++d) {
      if ((uint32_t)d >= r0) break;
      step(w[d], -s[d]);
    }
  }
  // ---- pass 2: the positives ascending, then the NaNs.  Every client is taken once in all, so
  // what step r takes stands at a position >= r: the last b steps lie above the window and are
  // not walked at all ----
  const uint32_t hi = m - a.trim;
  for (uint32_t r0 = 0u; r0 < hi; r0 += kSTDepth) {
    uint32_t w[kSTDepth];
    float s[kSTDepth];
#pragma unroll
    for (int d = 0; d < kSTDepth; ++d) {
      const uint32_t r = r0 + (uint32_t)d;
      w[d] = 0u; s[d] = 0.f;
      if (r < hi) {
        const STrimClient c = s_cl[r];
        if (r < nn) w[d] = ((const FC_G uint32_t*)c.words)[wi] ^ c.flip;
        s[d] = c.s;
      }
    }
#pragma unroll
    for (int d = 0; d < kSTDepth; ++d) {
      if (r0 + (uint32_t)d >= hi) break;
      step(~w[d], s[d]);
    }
  }
#pragma unroll
  for (int b = 0; b < 32; ++b) acc[b] = __fdiv_rn(acc[b], a.div);
  if (c0 + 32 <= a.n) {
#pragma unroll
    for (int b = 0; b < 32; b += 4)
      *(FC_G fc_f4v*)(a.out + c0 + b) = fc_f4v{acc[b], acc[b + 1], acc[b + 2], acc[b + 3]};
  } else {
#pragma unroll
    for (int b = 0; b < 32; ++b) if (c0 + b < a.n) a.out[c0 + b] = acc[b];
  }
}

}  // namespace fc

using namespace fc;

extern "C" {

size_t fc_sign_trim_workspace_bytes(uint64_t n, int m) {
  (void)n; (void)m;
  return 0;
}

int fc_sign_trim(const fc_packet_view* views_dev, int m, uint64_t n, int trim, float* out,
                 void* ws, size_t ws_bytes, fc_stream_t stream) {
  FC_CHECK(views_dev != nullptr, "views_dev is NULL");
  FC_CHECK(out != nullptr, "out is NULL");
  FC_CHECK(m >= 1 && m <= FC_GRAM_MAX_M, "m=%d outside [1, %d]", m, FC_GRAM_MAX_M);
  FC_CHECK(trim >= 0 && 2 * (int64_t)trim < (int64_t)m, "trim=%d outside [0, m/2) for m=%d", trim, m);
  FC_CHECK(n >= 1 && n <= 0xffffffffull, "n=%llu outside [1, 2^32-1]", (unsigned long long)n);
  FC_CHECK(((uintptr_t)out & 15) == 0, "out must be 16-byte aligned");
  FC_CHECK(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
  const size_t need = fc_sign_trim_workspace_bytes(n, m);
  FC_CHECK(ws != nullptr || need == 0, "workspace is NULL");
  if (ws_bytes < need)
    return fail(FC_ERR_WORKSPACE, "workspace %zu B < %zu B needed", ws_bytes, need);
  STrimArgs a;
  memset(&a, 0, sizeof a);
  a.views = views_dev; a.out = out; a.n = n; a.n_words = sign_words(n);
  a.m = (uint32_t)m; a.trim = (uint32_t)trim; a.span = (uint32_t)(m - 2 * trim);
  a.div = (float)(m - 2 * trim);
  const dim3 grid((uint32_t)((a.n_words + kBlock - 1) / kBlock)), blk(kBlock);
  hipLaunchKernelGGL(k_sign_trim, grid, blk, 0, (hipStream_t)stream, a);
  FC_LAUNCHED("k_sign_trim");
  return FC_OK;
}

}  // extern "C"
