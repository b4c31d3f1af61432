// fc_dot.hip — a round's packets times a dense vector, in float64, for MI355X (gfx950).
//
// out[i] = sum_t (double)d_i[t] * (double)v[t] for the m clients, d_i the float32 row
// fc_packets_gram uses (gram_rule / gram_value / gram_range of fc_gram.hip, not restated), and
// out[m] = sum_t (double)v[t]^2.  v == NULL stands for the all-ones vector: out[i] is the row
// sum and out[m] = (double)n.  The dense M x N matrix G is never built.
//
// k_dot, workgroup (tile, slice): the tile is kVTile = 64 consecutive clients (wave w takes the
// tile's clients w, w + 8, ...), the slice a range of chunks that depends on n and m alone.  For
// every chunk of its slice the workgroup
//   1. loads v's 8192 floats of the chunk into LDS with coalesced 16-B loads (32 KiB, zeros past
//      n; no scatter, nothing to clear afterwards).  Tile 0 also adds the squares of what it
//      loads into a per-thread float64 sum.  Skipped when v == NULL;
//   2. streams every client's entries of the chunk: lane l takes entries l + 64 r in order,
//      kVR rounds of loads in flight, reads v at the entry's location from LDS and adds the
//      exact product into ONE per-lane float64 accumulator per (client, chunk);
//   3. sums the accumulator over the wave by a fixed butterfly and adds it to the client's
//      float64 sum in LDS (owned by the client's wave, chunks in order).
// After its slice the workgroup stores its clients' sums and non-finite flags, and tile 0 its
// sum of squares, to ITS part of the workspace.  k_dot_fin (one wave per output) adds the parts:
// lane l those of slices l, l + 64, ... in order, then the same butterfly.  A flagged client's
// output is NaN; a non-finite sum of squares (v holds a NaN or an inf: the squares of finite
// float32 cannot overflow float64) makes every output NaN.  No floating-point atomics, no
// workgroup waits for another, and every workspace word that is read was written by the same
// call (no zeroing).  Every sum starts from +0.0.
//
// Why a whole chunk per image and not k_gram's quarter: v is dense, so its image is 4 bytes per
// coordinate whatever the tile holds (k_gram's is 4 * kGT) and 32 KiB leaves LDS for four workgroups per
// CU (kVSlices); a client's entries of a chunk then fill the wave's rounds (at f = 0.1 about 820 entries:
// 13 rounds, 1.5 % idle lanes, against 4 x 4 rounds a fifth idle by quarters) and the wave
// reduction comes once per (client, chunk), not once per quarter.  The quarter an entry is
// listed under still has to match its index, as in k_gram: it is found from the entry's
// position and the chunk's three inner quarter offsets (ascending, as every encoder writes them).
#include "fc_state.h"

namespace fc {

constexpr int kVBlock = 512;
constexpr int kVWaves = kVBlock / 64;
constexpr int kVTile = 64;                        // clients per workgroup: up to 8 per wave
constexpr int kVR = 4;                            // rounds (x 64 lanes) of entry loads in flight
constexpr uint32_t kVSlices = 1024;               // tiles x slices at most: four workgroups per CU
constexpr int kVStride = kGMaxM;                  // clients per slice row of the workspace
static_assert(kVTile % kVWaves == 0 && kGMaxM % kVTile == 0, "tile geometry");
static_assert(kChunk % (4 * kVBlock) == 0, "the image is loaded in whole float4 rounds");

struct DotArgs {
  const fc_packet_view* views;                    // DEVICE array of m views
  const float* v;                                 // DEVICE float32[n], or nullptr: all ones
  double* part;                                   // [slices][kVStride] per-client partial sums
  uint32_t* bad;                                  // [slices][kVStride] non-finite flags
  double* qpart;                                  // [slices] partial sums of v's squares
  double* out;                                    // [m + 1]
  uint64_t n;
  uint32_t m;
  uint32_t nch, cps, slices;                      // chunks; chunks per slice; slices launched
};

// The sum of x over the wave's 64 lanes, in every lane: a fixed butterfly (IEEE addition is
// commutative, so both lanes of a pair get the same bits at every step).
__device__ __forceinline__ double dot_wave_sum(double x) {
#pragma unroll
  for (int mask = 32; mask >= 1; mask >>= 1) x = x + __shfl_xor(x, mask, 64);
  return x;
}

// Eight waves per SIMD asked for: the stream is latency-bound, and four resident workgroups per CU
// at 64 VGPRs (three of them spilt, 16 bytes of scratch) measured 17 % / 10 % faster at 128 x 16 M /
// 32 x 128 M than three at the 68 VGPRs the kernel takes unasked.
__global__ __launch_bounds__(kVBlock, 8) void k_dot(DotArgs a) {
  __shared__ __attribute__((aligned(16))) float img[kChunk];   // v's floats of the chunk
  __shared__ GramMeta meta[kVTile];
  __shared__ uint64_t sqo[kVTile];
  __shared__ double blk[kVTile];
  __shared__ double swq[kVWaves];
  __shared__ uint32_t sbad[kVTile / 32];
  const int tid = threadIdx.x, lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t tile0 = blockIdx.x * kVTile, slice = blockIdx.y;
  const uint32_t tn = min(a.m - tile0, (uint32_t)kVTile);       // clients of this tile (>= 1)
  const uint32_t c0 = slice * a.cps, c1 = min(c0 + a.cps, a.nch);
  const bool dense = a.v != nullptr;                             // uniform
  const bool squares = dense && blockIdx.x == 0;                 // uniform

  if (tid < kVTile) blk[tid] = 0.0;
  if (tid < kVTile / 32) sbad[tid] = 0u;
  if ((uint32_t)tid < tn) meta[tid] = gram_meta(a.views[tile0 + tid]);
  double q = 0.0;

  typedef __attribute__((address_space(1))) const uint64_t gu64;
  for (uint32_t c = c0; c < c1; ++c) {
    const uint64_t base = (uint64_t)c * kChunk;
    __syncthreads();                               // the previous chunk's image and offsets are done with
    if ((uint32_t)tid < tn) sqo[tid] = ((gu64*)meta[tid].qoff)[c];
    if (dense) {
      // ---- 1. v's chunk into the image; nothing of v is read at or past n ----
#pragma unroll
      for (int i = tid; i < kChunk / 4; i += kVBlock) {
        const uint64_t t = base + 4ull * (uint32_t)i;
        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t + 4 <= a.n) {
          f = *reinterpret_cast<const float4*>(a.v + t);
        } else {
          if (t < a.n) f.x = a.v[t];
          if (t + 1 < a.n) f.y = a.v[t + 1];
          if (t + 2 < a.n) f.z = a.v[t + 2];
        }
        reinterpret_cast<float4*>(img)[i] = f;
        if (squares) {
          q = fma((double)f.x, (double)f.x, q); q = fma((double)f.y, (double)f.y, q);
          q = fma((double)f.z, (double)f.z, q); q = fma((double)f.w, (double)f.w, q);
        }
      }
    }
    __syncthreads();
    // ---- 2. + 3. wave w streams the tile's clients w, w + 8, ... against the image ----
    for (uint32_t t = (uint32_t)w; t < tn; t += kVWaves) {      // uniform per wave
      const uint64_t qo = uni64(sqo[t]);
      uint32_t s_, b0, b1, b2, en;
      gram_range(qo, 0, &s_, &b0);
      gram_range(qo, 1, &s_, &b1);
      gram_range(qo, 2, &s_, &b2);
      gram_range(qo, 3, &s_, &en);                 // entries [0, en) of the slot, en <= kChunk
      if (en == 0) continue;                       // uniform: the client lists nothing here
      const GramMeta& pm = meta[t];
      const GramRule r = gram_rule(pm, base);
      gu16* pidx = (gu16*)uni_ptr(pm.idx) + base;
      gf32* pval = (gf32*)uni_ptr(pm.val) + base;
      const uint32_t last = en - 1u;               // lanes past the end re-read the last entry
      double acc = 0.0;
      bool nonfinite = false;
      for (uint32_t e0 = 0; e0 < en; e0 += (uint32_t)(kVR * 64)) {
        uint32_t lcs[kVR];
        float vs[kVR];
#pragma unroll
        for (int rr = 0; rr < kVR; ++rr) {
          const uint32_t e = min(e0 + (uint32_t)(lane + rr * 64), last);
          lcs[rr] = pidx[e];
          vs[rr] = pval[e];
        }
#pragma unroll
        for (int rr = 0; rr < kVR; ++rr) {
          const uint32_t e = e0 + (uint32_t)(lane + rr * 64);
          const uint32_t lc = lcs[rr];
          const uint32_t qe = (uint32_t)(e >= b0) + (uint32_t)(e >= b1) + (uint32_t)(e >= b2);
          float x;
          const bool ok = (e < en) & gram_value(r, base, lc, vs[rr], &x) & ((lc >> 11) == qe);
          nonfinite |= ok & ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u);
          // a lane with nothing to add adds zero (times location 0 of the image); ok implies
          // lc >> 11 <= 3: the location is inside the image
          const double xd = ok ? (double)x : 0.0;
          if (dense) acc = fma(xd, (double)img[ok ? lc : 0u], acc);
          else acc = acc + xd;
        }
      }
      const double s = dot_wave_sum(acc);
      if (lane == 0) blk[t] += s;                  // t is this wave's alone, chunks in order
      if (nonfinite) atomicOr(&sbad[t >> 5], 1u << (t & 31u));
    }
  }
  __syncthreads();
  // ---- this workgroup's part ----
  if ((uint32_t)tid < tn) {
    const uint64_t o = (uint64_t)slice * kVStride + tile0 + (uint32_t)tid;
    a.part[o] = blk[tid];
    a.bad[o] = ((sbad[tid >> 5] >> (tid & 31)) & 1u) | ((meta[tid].flags & kGDead) ? 1u : 0u);
  }
  if (squares) {                                   // uniform per workgroup
    const double s = dot_wave_sum(q);
    if (lane == 0) swq[w] = s;
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
#pragma unroll
      for (int i = 0; i < kVWaves; ++i) t = t + swq[i];
      a.qpart[slice] = t;
    }
  }
}

// One wave per output: out[i] (i < m) = client i's parts added (lane l: slices l, l + 64, ... in
// order, then the butterfly), NaN when a part flags the client or v is not finite; out[m] = the
// sum of v's squares added the same way, or (double)n for the all-ones vector.
__global__ __launch_bounds__(64) void k_dot_fin(DotArgs a) {
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  const bool dense = a.v != nullptr;
  double q = 0.0, s = 0.0;
  uint32_t bad = 0;
  if (dense)
    for (uint32_t sl = lane; sl < a.slices; sl += 64) q = q + a.qpart[sl];
  q = dense ? dot_wave_sum(q) : (double)a.n;
  if (i < a.m) {
    for (uint32_t sl = lane; sl < a.slices; sl += 64) {
      s = s + a.part[(uint64_t)sl * kVStride + i];
      bad |= a.bad[(uint64_t)sl * kVStride + i];
    }
    s = dot_wave_sum(s);
  } else {
    s = q;
  }
#pragma unroll
  for (int mask = 32; mask >= 1; mask >>= 1) bad |= (uint32_t)__shfl_xor((int)bad, mask, 64);
  const bool vbad = (__double_as_longlong(q) & 0x7ff0000000000000ll) == 0x7ff0000000000000ll;
  if (bad || vbad) s = __longlong_as_double(0x7ff8000000000000ll);
  if (lane == 0) a.out[i] = s;
}

}  // namespace fc
