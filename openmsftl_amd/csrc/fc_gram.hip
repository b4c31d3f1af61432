// fc_gram.hip — the M x M Gram matrix G G^T of a round's packets, in float64, for MI355X (gfx950).
//
// gram[i][j] = sum_t (double)d_i[t] * (double)d_j[t], d_i the float32 row fc_decode_dense makes of
// packet i (FC_FMT_IDXVAL with quarter offsets).  The dense M x N matrix G is never built: the
// work is sparse x dense-tile, one chunk quarter (2048 coordinates) at a time.
//
// k_gram, workgroup (tile, slice): the tile is kGT = 8 consecutive clients, the slice a range of
// chunks that depends on n and m alone.  For every quarter of its chunks the workgroup
//   1. scatters the kept entries of the tile's clients into an LDS image [2048][kGT] floats
//      (64 KiB; one wave per tile client), flagging a client whose kept value is not finite;
//   2. streams the quarter's entries of every client j >= the tile's first client against it,
//      wave w taking j = first + w, first + w + 8, ...: a lane takes an entry (loc, v), reads the
//      image's kGT floats at loc (two 16-B LDS reads) and adds (double)v * (double)image[t] into
//      kGT per-lane float64 accumulators.  The products of two float32 are exact in float64;
//   3. reduces the kGT accumulators across the wave TOGETHER (the values a lane holds halve as
//      the lane span halves: 4 + 2 + 1 + 3 adds, not 6 per accumulator) and adds the sums into
//      the workgroup's [kGT][M] float64 block in LDS.  Entry (t, j) of the block is owned by
//      j's wave and quarters come in order, so the order of summation is fixed;
//   4. zeroes the image slots it wrote again (k stores, not 2048 * kGT).
// After its slice the workgroup stores the block and its clients' flags to ITS part of the
// workspace.  k_gram_fin adds the parts in slice order, mirrors the upper triangle and writes NaN
// into the rows and columns of flagged clients.  No floating-point atomics, no workgroup waits
// for another, and every workspace word that is read was written by the same call (no zeroing).
//
// Why kGT = 8: the image costs 2048 * kGT * 4 bytes, 64 KiB of a CU's 160 KiB, and an entry of the
// stream does kGT multiply-adds per 4 * kGT bytes read from LDS whatever kGT is, so a wider tile
// saves only global reads of the stream (which L2 serves) at half the resident waves.
#include "fc_state.h"

namespace fc {

constexpr int FC_GRAM_TILE = 8;
constexpr int kGT = FC_GRAM_TILE;                 // clients per tile
constexpr int kGBlock = 512;                      // 8 waves: one per tile client in the scatter
constexpr int kGWaves = kGBlock / 64;
constexpr int kGMaxM = 128;                       // FC_GRAM_MAX_M
constexpr int kGR = 4;                            // register rounds (x 64 lanes) per (client, quarter)
constexpr uint32_t kGSlices = 2048;               // tiles (rounded up to a power of two) x slices
constexpr int kGQuarter = kChunk / 4;
static_assert(kGT == 8, "the wave reduction halves 8 accumulators");
static_assert(kGWaves == kGT, "wave w scatters tile client w");

struct GramMeta {                                 // one packet, staged in LDS once per workgroup
  const void* idx;                                // uint16 chunk-local indices
  const float* val;
  const uint64_t* qoff;
  const fc_packet_hdr* hdr;
  uint64_t thresh;
  uint32_t flags;                                 // ib | codec << 8 | key_mode << 16 | kGGeneric | kGDead
  uint32_t pad_;
};
static_assert(sizeof(GramMeta) == 48, "GramMeta layout");
constexpr uint32_t kGGeneric = 1u << 24;          // per-entry rules: Philox keys, 1/p scaling, T64 at inf
constexpr uint32_t kGDead = 1u << 25;             // dropout-unbiased with p == 0: the row is all NaN

constexpr size_t kGLdsImg = (size_t)kGQuarter * kGT * 4;                 // 65536
constexpr size_t kGLdsBlk = (size_t)kGT * kGMaxM * 8;                    // 8192
constexpr size_t kGLdsMeta = (size_t)kGMaxM * sizeof(GramMeta);          // 6144
constexpr size_t kGLdsQo = (size_t)kGMaxM * 8;                           // 1024
constexpr size_t kGLdsBytes = kGLdsImg + kGLdsBlk + kGLdsMeta + kGLdsQo + 16;

struct GramArgs {
  const fc_packet_view* views;                    // DEVICE array of m views
  double* part;                                   // [slices][mp][mp] partial Grams (upper triangle)
  uint32_t* bad;                                  // [slices][mp] non-finite flags
  double* gram;                                   // [m][m]
  uint64_t n;
  uint32_t m, mp;                                 // clients; row stride of a part
  uint32_t nch, cps, slices;                      // chunks; chunks per slice; slices launched
};

// One packet's GramMeta from its view (reads the packet's device header).
__device__ __forceinline__ GramMeta gram_meta(const fc_packet_view& v) {
  const fc_packet_hdr* h = v.hdr;
  GramMeta d;
  d.idx = v.idx; d.val = v.val; d.qoff = v.qoff; d.hdr = h; d.thresh = h->thresh; d.pad_ = 0;
  const uint32_t ib = h->index_bits & 0xffu, codec = h->codec, key_mode = h->key_mode;
  const bool unb = codec == FC_CODEC_DROPOUT_UNBIASED;
  const bool generic = unb || (key_mode == FC_KEY_PHILOX && d.thresh != 0) ||
                       (d.thresh >> ib) >= 0x7f800000ull;
  d.flags = ib | ((codec & 0xffu) << 8) | ((key_mode & 0xffu) << 16) |
            (generic ? kGGeneric : 0u) | ((unb && h->p == 0.0) ? kGDead : 0u);
  return d;
}

// The per-(client, chunk) constants of the keep rule (wave-uniform).
struct GramRule {
  PktCache pk;                                    // generic: entry_kept + fl32(fl64(v)/p)
  float Tf;                                       // fast form: T64's key as a float
  uint32_t Tr;                                    //            and its index cut inside the chunk
  bool generic;
};

__device__ __forceinline__ GramRule gram_rule(const GramMeta& pm, uint64_t base) {
  GramRule r;
  const uint32_t flags = uni32(pm.flags);
  const uint64_t thresh = uni64(pm.thresh);
  const uint32_t ib = flags & 0xffu;
  r.generic = (flags & kGGeneric) != 0;
  r.pk.thresh = thresh; r.pk.ib = ib;
  r.pk.codec = (flags >> 8) & 0xffu; r.pk.key_mode = (flags >> 16) & 0xffu;
  r.pk.seed = 0; r.pk.offset = 0; r.pk.p = 1.0;
  if (r.generic) {
    const fc_packet_hdr* h = (const fc_packet_hdr*)uni_ptr(pm.hdr);
    r.pk.seed = h->seed; r.pk.offset = h->offset; r.pk.p = h->p;
  }
  r.Tf = __uint_as_float((uint32_t)(thresh >> ib));
  const uint32_t Ti = (uint32_t)(thresh & ((1ull << ib) - 1ull));
  const uint32_t b32 = (uint32_t)base;
  r.Tr = Ti <= b32 ? 0u : min(Ti - b32, (uint32_t)kChunk);
  return r;
}

// d_i's value for a listed entry (chunk-local lc, value v); false: the entry is slack.
__device__ __forceinline__ bool gram_value(const GramRule& r, uint64_t base, uint32_t lc, float v,
                                           float* x) {
  if (r.generic) {
    if (!entry_kept(r.pk, (uint32_t)base + lc, v)) return false;
    *x = kept_f32(v, r.pk);
    return true;
  }
  // comp >= T64  <=>  !(|v| <= Tf) || (|v| == Tf && lc >= Tr)   (see k_fold_q)
  const float av = __builtin_fabsf(v);
  *x = v;
  return !(av <= r.Tf) | ((av == r.Tf) & (lc >= r.Tr));
}

__device__ __forceinline__ void gram_range(uint64_t qo, int q, uint32_t* st, uint32_t* en) {
  uint32_t s, e;
  quarter_range(qo, q, &s, &e);
  e = min(e, (uint32_t)kChunk);                   // never outside the chunk's slot
  *st = min(s, e); *en = e;
}

__device__ __forceinline__ double gram_shx(double v, int mask) { return __shfl_xor(v, mask, 64); }
// The same value moved inside a row of 16 lanes by a DPP control (no LDS crossbar round trip):
// 0x128 row_ror:8 (lane ^ 8), 0x141 row_half_mirror (7 - lane within 8), 0x4E / 0xB1 quad_perm
// [2,3,0,1] / [1,0,3,2] (lane ^ 2, lane ^ 1).
template <int CTRL>
__device__ __forceinline__ double gram_dpp(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// Sum each of the 8 accumulators over the wave's 64 lanes: after the call the first lane of the
// group lane >> 3 holds the sum of accumulator *t = lane >> 3 (the group's other lanes hold the
// same sum associated in another order: only the first lane's is used).  A fixed tree: the same
// inputs give the same bits.
__device__ __forceinline__ double gram_reduce8(const double* acc, int lane, int* t) {
  const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;
  double a4[4], a2[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double keep = b5 ? acc[4 + i] : acc[i], give = b5 ? acc[i] : acc[4 + i];
    a4[i] = keep + gram_shx(give, 32);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double keep = b4 ? a4[2 + i] : a4[i], give = b4 ? a4[i] : a4[2 + i];
    a2[i] = keep + gram_shx(give, 16);
  }
  const double keep = b3 ? a2[1] : a2[0], give = b3 ? a2[0] : a2[1];
  double r = keep + gram_dpp<0x128>(give);
  // the eight lanes of a group now hold eight partial sums of one accumulator: lane 0 of the
  // group adds them as ((x0 + x7) + (x1 + x6)) + ((x2 + x5) + (x3 + x4))
  r = r + gram_dpp<0x141>(r);
  r = r + gram_dpp<0xB1>(r);
  r = r + gram_dpp<0x4E>(r);
  *t = (b5 ? 4 : 0) | (b4 ? 2 : 0) | (b3 ? 1 : 0);
  return r;
}

__global__ __launch_bounds__(kGBlock, 1) void k_gram(GramArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char g_lds[];
  float* img = reinterpret_cast<float*>(g_lds);                               // [2048][kGT]
  double* blk = reinterpret_cast<double*>(g_lds + kGLdsImg);                  // [kGT][kGMaxM]
  GramMeta* meta = reinterpret_cast<GramMeta*>(g_lds + kGLdsImg + kGLdsBlk);  // [kGMaxM]
  uint64_t* sqo = reinterpret_cast<uint64_t*>(g_lds + kGLdsImg + kGLdsBlk + kGLdsMeta);
  uint32_t* sbad = reinterpret_cast<uint32_t*>(g_lds + kGLdsImg + kGLdsBlk + kGLdsMeta + kGLdsQo);
  const int tid = threadIdx.x, lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t M = a.m;
  const uint32_t tile0 = blockIdx.x * kGT, slice = blockIdx.y;
  const uint32_t c0 = slice * a.cps, c1 = min(c0 + a.cps, a.nch);

  for (int i = tid; i < kGQuarter * kGT / 4; i += kGBlock)
    reinterpret_cast<float4*>(img)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = tid; i < kGT * kGMaxM; i += kGBlock) blk[i] = 0.0;
  if (tid == 0) *sbad = 0u;
  if ((uint32_t)tid < M) {
    meta[tid] = gram_meta(a.views[tid]);
  }
  __syncthreads();

  typedef __attribute__((address_space(1))) const uint64_t gu64;
  for (uint32_t c = c0; c < c1; ++c) {
    const uint64_t base = (uint64_t)c * kChunk;
    __syncthreads();                               // the previous chunk's offsets are done with
    if ((uint32_t)tid < M) sqo[tid] = ((gu64*)meta[tid].qoff)[c];
    __syncthreads();
    for (int q = 0; q < 4; ++q) {
      // a quarter in which the tile's clients list nothing adds nothing (uniform)
      uint32_t tile_n = 0;
      for (int t = 0; t < kGT; ++t) {
        if (tile0 + t >= M) break;
        uint32_t st, en;
        gram_range(uni64(sqo[tile0 + t]), q, &st, &en);
        tile_n += en - st;
      }
      if (tile_n == 0) continue;
      // ---- 1. the tile's kept entries into the image: wave w scatters tile client w.  The
      // first kGR * 64 entries come in unconditional rounds (one load latency, not one per
      // round); the image slots written are kept for step 4 ----
      const uint32_t ti = tile0 + (uint32_t)w;
      uint32_t clr[kGR];
      uint32_t cst = 0, cen = 0;
#pragma unroll
      for (int rr = 0; rr < kGR; ++rr) clr[rr] = ~0u;
      if (ti < M) {                                  // uniform per wave
        gram_range(uni64(sqo[ti]), q, &cst, &cen);
        const GramMeta& pm = meta[ti];
        const GramRule r = gram_rule(pm, base);
        gu16* pidx = (gu16*)uni_ptr(pm.idx) + base;
        gf32* pval = (gf32*)uni_ptr(pm.val) + base;
        const uint32_t cnt = cen - cst;
        const uint32_t last = min(cst + (cnt ? cnt - 1u : 0u), (uint32_t)(kChunk - 1));
        uint32_t lc4[kGR];
        float v4[kGR];
#pragma unroll
        for (int rr = 0; rr < kGR; ++rr) {
          const uint32_t e = min(cst + (uint32_t)(lane + rr * 64), last);
          lc4[rr] = pidx[e];
          v4[rr] = pval[e];
        }
        bool nonfinite = false;
        const int lim = (int)cnt - lane;
#pragma unroll
        for (int rr = 0; rr < kGR; ++rr) {
          float x;
          if ((lim > rr * 64) && gram_value(r, base, lc4[rr], v4[rr], &x) &&
              (lc4[rr] >> 11) == (uint32_t)q) {
            clr[rr] = (lc4[rr] & (uint32_t)(kGQuarter - 1)) * kGT + (uint32_t)w;
            img[clr[rr]] = x;
            nonfinite |= (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
          }
        }
        for (uint32_t e = cst + (uint32_t)(kGR * 64 + lane); e < cen; e += 64) {   // a long quarter
          const uint32_t lc = pidx[e];
          float x;
          if (gram_value(r, base, lc, pval[e], &x) && (lc >> 11) == (uint32_t)q) {
            img[(lc & (uint32_t)(kGQuarter - 1)) * kGT + w] = x;
            nonfinite |= (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
          }
        }
        if (nonfinite) atomicOr(sbad, 1u << w);
      }
      __syncthreads();
      // ---- 2. + 3. every client from the tile's first one on, streamed against the image ----
      {
        // three register slots: the loads of two clients in flight while a third is folded
        uint32_t lcs[3][kGR];
        float vs[3][kGR];
        uint32_t sst[3], sen[3];
        auto issue = [&](int sl, uint32_t j) {
          j = min(j, M - 1);                      // past the end: re-load (ignored)
          gram_range(uni64(sqo[j]), q, &sst[sl], &sen[sl]);
          const GramMeta& pm = meta[j];
          gu16* pidx = (gu16*)uni_ptr(pm.idx) + base;
          gf32* pval = (gf32*)uni_ptr(pm.val) + base;
          // lanes past the range's end re-read its last entry; an empty range reads one entry
          // of the slot (ignored).  Every position stays inside the chunk's slot of 8192.
          const uint32_t cnt = sen[sl] - sst[sl];
          const uint32_t last = min(sst[sl] + (cnt ? cnt - 1u : 0u), (uint32_t)(kChunk - 1));
#pragma unroll
          for (int r = 0; r < kGR; ++r) {
            const uint32_t e = min(sst[sl] + (uint32_t)(lane + r * 64), last);
            lcs[sl][r] = pidx[e];
            vs[sl][r] = pval[e];
          }
        };
        auto process = [&](int sl, uint32_t j) {
          const uint32_t st = sst[sl], en = sen[sl];
          if (en == st) return;                   // uniform: nothing to add for (tile, j, quarter)
          const GramMeta& pm = meta[j];
          const GramRule r = gram_rule(pm, base);
          double acc[kGT];
#pragma unroll
          for (int t = 0; t < kGT; ++t) acc[t] = 0.0;
          auto add = [&](uint32_t loc, double xd) {
            const float4 i0 = *reinterpret_cast<const float4*>(&img[loc * kGT]);
            const float4 i1 = *reinterpret_cast<const float4*>(&img[loc * kGT + 4]);
            acc[0] = fma(xd, (double)i0.x, acc[0]); acc[1] = fma(xd, (double)i0.y, acc[1]);
            acc[2] = fma(xd, (double)i0.z, acc[2]); acc[3] = fma(xd, (double)i0.w, acc[3]);
            acc[4] = fma(xd, (double)i1.x, acc[4]); acc[5] = fma(xd, (double)i1.y, acc[5]);
            acc[6] = fma(xd, (double)i1.z, acc[6]); acc[7] = fma(xd, (double)i1.w, acc[7]);
          };
          if (!r.generic) {
            const int lim = (int)(en - st) - lane;
#pragma unroll
            for (int rr = 0; rr < kGR; ++rr) {
              if (en - st <= (uint32_t)(rr * 64)) break;        // uniform: no lane has an entry
              const uint32_t lc = lcs[sl][rr];
              float x;
              const bool ok = (lim > rr * 64) & gram_value(r, base, lc, vs[sl][rr], &x) &
                              ((lc >> 11) == (uint32_t)q);
              // a lane with nothing to add multiplies location 0 by zero
              add(ok ? lc & (uint32_t)(kGQuarter - 1) : 0u, ok ? (double)x : 0.0);
            }
          }
          const uint32_t e0 = r.generic ? st : st + (uint32_t)(kGR * 64);
          if (e0 < en) {                          // uniform: the per-entry rules, or a long quarter
            gu16* pidx = (gu16*)uni_ptr(pm.idx) + base;
            gf32* pval = (gf32*)uni_ptr(pm.val) + base;
            for (uint32_t e = e0 + (uint32_t)lane; e < en; e += 64) {
              const uint32_t lc = pidx[e];
              float x;
              if (gram_value(r, base, lc, pval[e], &x) && (lc >> 11) == (uint32_t)q)
                add(lc & (uint32_t)(kGQuarter - 1), (double)x);
            }
          }
          int t;
          const double s = gram_reduce8(acc, lane, &t);
          if ((lane & 7) == 0) blk[t * kGMaxM + j] += s;   // (t, j): this wave's, quarters in order
        };
        const uint32_t j0 = tile0 + (uint32_t)w;
        if (j0 < M) {                              // uniform per wave
          issue(0, j0);
          issue(1, j0 + kGWaves);
          for (uint32_t j = j0; j < M; j += 3 * kGWaves) {
            issue(2, j + 2 * kGWaves);
            process(0, j);
            if (j + kGWaves >= M) break;
            issue(0, j + 3 * kGWaves);
            process(1, j + kGWaves);
            if (j + 2 * kGWaves >= M) break;
            issue(1, j + 4 * kGWaves);
            process(2, j + 2 * kGWaves);
          }
        }
      }
      __syncthreads();
      // ---- 4. the image back to zero: the slots step 1 wrote, and a long quarter's rest ----
#pragma unroll
      for (int rr = 0; rr < kGR; ++rr)
        if (clr[rr] != ~0u) img[clr[rr]] = 0.f;
      if (cen - cst > (uint32_t)(kGR * 64)) {        // uniform per wave (ti < M)
        gu16* pidx = (gu16*)uni_ptr(meta[ti].idx) + base;
        for (uint32_t e = cst + (uint32_t)(kGR * 64 + lane); e < cen; e += 64)
          img[(pidx[e] & (uint32_t)(kGQuarter - 1)) * kGT + w] = 0.f;
      }
      // (no barrier: column t of the image is written by one wave only, here and in step 1)
    }
  }
  __syncthreads();
  // ---- this workgroup's part: rows of the tile, columns from the tile's first client on ----
  double* part = a.part + (uint64_t)slice * a.mp * a.mp;
  for (uint32_t i = (uint32_t)tid; i < (uint32_t)kGT * M; i += kGBlock) {
    const uint32_t t = i / M, j = i - t * M;
    if (tile0 + t < M && j >= tile0) part[(uint64_t)(tile0 + t) * a.mp + j] = blk[t * kGMaxM + j];
  }
  if (tid < kGT && tile0 + (uint32_t)tid < M)
    a.bad[(uint64_t)slice * a.mp + tile0 + tid] =
        ((*sbad >> tid) & 1u) | ((meta[tile0 + tid].flags & kGDead) ? 1u : 0u);
}

// gram[i][j] = gram[j][i] = the parts' (i, j) added in slice order, or NaN when client i or j holds
// a non-finite element.  One thread per (i, j), i <= j.
__global__ __launch_bounds__(kBlock) void k_gram_fin(GramArgs a) {
  const uint32_t M = a.m;
  const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= M * M) return;
  const uint32_t i = e / M, j = e - i * M;
  if (i > j) return;
  double s = 0.0;
  uint32_t bad = 0;
  for (uint32_t sl = 0; sl < a.slices; ++sl) {
    s = s + a.part[((uint64_t)sl * a.mp + i) * a.mp + j];
    bad |= a.bad[(uint64_t)sl * a.mp + i] | a.bad[(uint64_t)sl * a.mp + j];
  }
  if (bad) s = __longlong_as_double(0x7ff8000000000000ll);
  a.gram[(uint64_t)i * M + j] = s;
  a.gram[(uint64_t)j * M + i] = s;
}

}  // namespace fc
