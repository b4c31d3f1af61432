// fc_trim.hip — coordinate-wise trimmed mean (and median) of a round's packets for MI355X (gfx950).
//
// out[t] = the float32 mean of the M - 2b middle values of d_0[t] .. d_{M-1}[t], d_i the float32
// row fc_packets_gram uses (gram_rule / gram_value / gram_range of fc_gram.hip, not restated): the
// M values in np.sort's order (-inf first, -0.0 == +0.0, +inf after every finite value, every NaN
// after +inf), the b smallest and the b largest dropped, the rest added in ascending order from
// +0.0 with __fadd_rn and divided by float32(M - 2b) with __fdiv_rn.  b = (M - 1) / 2 is the
// median.  The dense M x N matrix G is never built and nothing of the packets is sorted but the
// non-zeros of a column: the implicit +0.0 of every packet that lists nothing at t form one block
// between the negatives and the positives.
//
// k_trim, one workgroup (512 threads) per chunk: the grid is a function of n alone.  The chunk is
// walked in windows of W coordinates (W = 256 up to 64 clients, 128 above: the [m][W] float tile
// in LDS is at most 64 KiB, two workgroups per CU).  Between windows the tile holds +0.0 (NaN in
// the row of a dropout-unbiased packet with p == 0, whose unlisted coordinates decode to NaN).
// For every window
//   1. the kept entries of the window go into the tile.  Entries ascend inside a quarter, so a
//      client's entries of the window are one run that starts at the client's cursor.  A wave's
//      lanes are groups of W / 8, a group per client (wave w: clients w, w + 8, ...): the group
//      reads W / 8 entries from the cursor on (issued during the previous window's steps 2 and
//      3), takes the leading ones below the window's end and moves the cursor past them; a run
//      of W / 8 or more goes round again.  One writer per cell: no LDS atomics;
//   2. after a barrier thread (g, c) owns rows [g R, g R + R) of column c, 512 / W row groups of
//      R = ceil(m / groups) <= 32 rows.  It reads down its rows (conflict-free in [m][W]), puts
//      every occupied cell back to its empty value, moves the non-zeros to the top of its
//      segment, counting the negatives, and insertion-sorts them there;
//   3. after a barrier one thread per column (W / 8 columns per wave, so that the short
//      divergent loops run on all four SIMDs) merges the column's sorted segments in ascending
//      order.  The rank window [b, M - b) lies over "negatives, M - nnz zeros, positives (NaN
//      last)"; a zero added to a sum that started from +0.0 never changes it, so the zero block
//      is only counted.  The merge adds what has a rank inside the window as it comes by, stops
//      at the window's end and puts the cells it used back to empty.  One 4-byte non-temporal
//      store per column, consecutive lanes consecutive addresses.
// No workspace, no floating-point atomics, no workgroup waits for another.  A malformed packet
// (entries that do not ascend, an entry listed under another quarter) loses entries as it does
// in fc_packets_gram, and never reaches outside the tile or the chunk's slot.
#include "fc_state.h"

namespace fc {

constexpr int kTBlock = 512;
constexpr int kTWaves = kTBlock / 64;
constexpr int kTIt = 4;                           // scatter rounds: (64 / (W / 8)) clients per wave each
constexpr int kTTile = 16384;                     // floats in the tile: 64 KiB
static_assert(kTIt * kTWaves * 4 >= kGMaxM && kTIt * kTWaves * 2 >= 64, "every client has a lane group");

__host__ __device__ constexpr uint32_t trim_window(uint32_t m) { return m > 64 ? 128u : 256u; }
static_assert(trim_window(kGMaxM) * kGMaxM <= kTTile && trim_window(64) * 64 <= kTTile, "tile size");
static_assert(kGQuarter % trim_window(1) == 0 && trim_window(kGMaxM) <= kTBlock &&
              trim_window(1) <= kTBlock, "a window lies in one quarter and has a thread per column");

struct TrimArgs {
  const fc_packet_view* views;                    // DEVICE array of m views
  float* out;                                     // [n]
  uint64_t n;
  uint32_t m, trim;
  float div;                                      // float32(m - 2 trim)
};

// d_i's value for a listed entry, gram_value (fc_gram.hip) with the client's rule per LANE: Tf / Tr
// are the fast form's constants of (client, chunk), made once per chunk.
__device__ __forceinline__ bool trim_value(const GramMeta& pm, float Tf, uint32_t Tr, uint64_t base,
                                           uint32_t lc, float v, float* x) {
  const uint32_t flags = pm.flags;
  if (flags & kGGeneric) {
    PktCache pk;
    pk.thresh = pm.thresh; pk.ib = flags & 0xffu;
    pk.codec = (flags >> 8) & 0xffu; pk.key_mode = (flags >> 16) & 0xffu;
    const fc_packet_hdr* h = pm.hdr;
    pk.seed = h->seed; pk.offset = h->offset; pk.p = h->p;
    if (!entry_kept(pk, (uint32_t)base + lc, v)) return false;
    *x = kept_f32(v, pk);
    return true;
  }
  const float av = __builtin_fabsf(v);
  *x = v;
  return !(av <= Tf) | ((av == Tf) & (lc >= Tr));
}

// a sorts after x: np.sort's order of two non-zeros, every NaN after every number
__device__ __forceinline__ bool trim_after(float a, float x) { return (a > x) | ((a != a) & (x == x)); }

__global__ __launch_bounds__(kTBlock, 4) void k_trim(TrimArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char t_lds[];
  float* tile = reinterpret_cast<float*>(t_lds);  // [m][W]
  __shared__ GramMeta meta[kGMaxM];
  __shared__ uint64_t sqo[kGMaxM];
  __shared__ uint32_t cur[kGMaxM];                // client i's cursor: owned by i's wave
  __shared__ float fill[kGMaxM];                  // the empty value of row i
  __shared__ float sTf[kGMaxM];                   // the keep rule's fast form for this chunk:
  __shared__ uint32_t sTr[kGMaxM];                // T64's key as a float, its index cut in the chunk
  __shared__ uint16_t scnt[4 * 256];              // [row group][column]: non-zeros | negatives << 8
  const int tid = threadIdx.x, lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t M = a.m, W = trim_window(M);
  const uint64_t base = (uint64_t)blockIdx.x * kChunk;
  const uint64_t left = a.n - base;               // > 0: the grid is the chunk count
  const uint32_t span = left < (uint64_t)kChunk ? (uint32_t)left : (uint32_t)kChunk;
  const uint32_t nwin = (span + W - 1) / W;

  typedef __attribute__((address_space(1))) const uint64_t gu64;
  int dead = 0;
  if ((uint32_t)tid < M) {
    const GramMeta pm = gram_meta(a.views[tid]);
    meta[tid] = pm;
    sqo[tid] = ((gu64*)pm.qoff)[blockIdx.x];
    cur[tid] = 0u;
    dead = (pm.flags & kGDead) != 0;
    fill[tid] = dead ? __uint_as_float(0x7fc00000u) : 0.f;
    const uint32_t ib = pm.flags & 0xffu;           // gram_rule's constants
    const uint32_t Ti = (uint32_t)(pm.thresh & ((1ull << ib) - 1ull));
    sTf[tid] = __uint_as_float((uint32_t)(pm.thresh >> ib));
    sTr[tid] = Ti <= (uint32_t)base ? 0u : min(Ti - (uint32_t)base, (uint32_t)kChunk);
  }
  const bool anydead = __syncthreads_or(dead) != 0;           // uniform; meta, sqo, fill are visible
  if (!anydead) {
    for (uint32_t i = (uint32_t)tid; i < M * W / 4; i += kTBlock)
      reinterpret_cast<float4*>(tile)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    for (uint32_t i = (uint32_t)tid; i < M * W; i += kTBlock) tile[i] = fill[i / W];
  }

  // Step 1's lanes: a wave's 64 lanes are 64 / LPG groups of LPG = W / 8 lanes, a group per client
  // (a window holds about f W entries of a client: a whole wave per client left four lanes in
  // five idle at f = 0.1 and paid the per-client bookkeeping 16 times per window).  Round it of
  // kTIt takes the wave's clients w + 8 (it GPW + sub), sub the lane's group.
  const uint32_t lsh = W == 128u ? 4u : 5u, LPG = 1u << lsh, GPW = 64u >> lsh;
  const uint32_t sub = (uint32_t)lane >> lsh, l = (uint32_t)lane & (LPG - 1u);
  uint32_t lcs[kTIt], cb[kTIt], ce[kTIt];
  float vs[kTIt];
  // the lane's clients: their run's start (the quarter's first slot at a quarter's first window,
  // the cursor otherwise) and end, and LPG entries from the start on.  Lanes past the slot's end
  // re-read its last entry (ignored: they are past the run's end too); a group without a client
  // reads client 0's (ignored).
  auto issue = [&](uint32_t win) {
    const uint32_t w0 = win * W;
    const int q = (int)(w0 >> 11);
    const bool first = (w0 & (uint32_t)(kGQuarter - 1)) == 0u;
#pragma unroll
    for (int it = 0; it < kTIt; ++it) {
      const uint32_t ir = (uint32_t)w + (uint32_t)kTWaves * ((uint32_t)it * GPW + sub);
      const uint32_t i = ir < M ? ir : 0u;
      uint32_t st, en;
      gram_range(sqo[i], q, &st, &en);
      const uint32_t c = first ? st : min(max(cur[i], st), en);
      cb[it] = c; ce[it] = en;
      gu16* pidx = (gu16*)meta[i].idx + base;
      gf32* pval = (gf32*)meta[i].val + base;
      const uint32_t e = min(c + l, (uint32_t)(kChunk - 1));
      lcs[it] = pidx[e];
      vs[it] = pval[e];
    }
  };
  auto scatter = [&](uint32_t win) {
    const uint32_t w0 = win * W, w1 = w0 + W;
#pragma unroll
    for (int it = 0; it < kTIt; ++it) {
      const uint32_t ir = (uint32_t)w + (uint32_t)kTWaves * ((uint32_t)it * GPW + sub);
      if ((uint32_t)w + (uint32_t)kTWaves * (uint32_t)it * GPW >= M) break;   // uniform: no group has a client
      const bool valid = ir < M;
      const uint32_t i = valid ? ir : 0u;
      const GramMeta& pm = meta[i];
      float* row = tile + i * W;
      const uint32_t en = ce[it];
      uint32_t c = cb[it], lc = lcs[it];
      float v = vs[it];
      bool act = valid;
      for (;;) {
        // the run's entries among the group's LPG: the leading ones below the window's end
        const bool in = act & (c + l < en) & (lc < w1);
        const uint64_t stop = __ballot(!in);
        const uint32_t cnt = (uint32_t)__builtin_ctzll((stop >> (sub * LPG)) | (1ull << LPG));
        float x;
        if (in && l < cnt && lc >= w0 && trim_value(pm, sTf[i], sTr[i], base, lc, v, &x)) row[lc - w0] = x;
        c += act ? cnt : 0u;
        act = act & (cnt == LPG);
        if (__ballot(act) == 0ull) break;          // uniform
        if (act) {                                 // a run of LPG or more: the group goes round again
          gu16* pidx = (gu16*)pm.idx + base;
          gf32* pval = (gf32*)pm.val + base;
          const uint32_t e = min(c + l, (uint32_t)(kChunk - 1));
          lc = pidx[e];
          v = pval[e];
        }
      }
      if (valid && l == 0u) cur[i] = c;
    }
  };

  const uint32_t b = a.trim, hi = M - b;
  // step 2's threads: kTBlock / W row groups of R rows; thread (g, c) owns rows [r0, r1) of column c
  const uint32_t G = (uint32_t)kTBlock / W, R = (M + G - 1) / G;
  const uint32_t sg = (uint32_t)tid / W, sc = (uint32_t)tid & (W - 1u);
  const uint32_t r0 = min(sg * R, M), r1 = min(r0 + R, M);
  // step 3's threads: every wave takes W / 8 columns (short divergent loops on all four SIMDs)
  const uint32_t mper = W / (uint32_t)kTWaves;
  const uint32_t mc = (uint32_t)w * mper + (uint32_t)lane;
  const bool merges = (uint32_t)lane < mper;
  issue(0);
  __syncthreads();                                 // the tile is empty
  for (uint32_t win = 0; win < nwin; ++win) {
    scatter(win);
    __syncthreads();
    if (win + 1 < nwin) issue(win + 1);            // in flight during the columns
    {
      // ---- 2. the non-zeros of rows [r0, r1) to the top of the segment, then sorted ----
      float* col = tile + sc;
      uint32_t cnt = 0, nneg = 0;
      for (uint32_t i0 = r0; i0 < r1; i0 += 4) {
        float x4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x4[u] = col[min(i0 + (uint32_t)u, r1 - 1u) * W];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const uint32_t i = i0 + (uint32_t)u;
          const float x = x4[u];
          if (i < r1 && __float_as_uint(x) != 0u) {
            col[i * W] = anydead ? fill[i] : 0.f;
            if (x != 0.f) {                        // (a kept -0.0 is one of the zero block)
              col[(r0 + cnt) * W] = x;             // r0 + cnt <= i
              ++cnt;
              nneg += x < 0.f ? 1u : 0u;
            }
          }
        }
      }
      float* seg = col + r0 * W;
      for (uint32_t e = 1; e < cnt; ++e) {
        const float x = seg[e * W];
        uint32_t j = e;
        while (j > 0) {
          const float p = seg[(j - 1) * W];
          if (!trim_after(p, x)) break;
          seg[j * W] = p;
          --j;
        }
        seg[j * W] = x;
      }
      scnt[sg * 256u + sc] = (uint16_t)(cnt | (nneg << 8));
    }
    __syncthreads();
    if (merges) {
      // ---- 3. the segments of column mc merged in ascending order; the ranks [b, hi) of
      // "negatives, M - nnz zeros, positives" are added as they come by ----
      float* col = tile + mc;
      uint32_t hp[4], he[4], total = 0, nneg = 0;
      float hv[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const uint32_t cn = (uint32_t)g < G ? (uint32_t)scnt[g * 256 + mc] : 0u;
        hp[g] = min((uint32_t)g * R, M);
        he[g] = hp[g] + (cn & 0xffu);
        total += cn & 0xffu;
        nneg += cn >> 8;
        hv[g] = col[min(hp[g], M - 1u) * W];
      }
      const uint32_t nz = M - total;
      float acc = 0.f;
      for (uint32_t k = 0; k < total; ++k) {
        const uint32_t rank = k < nneg ? k : k + nz;
        if (rank >= hi) break;
        int best = -1;
        float bv = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g)
          if (hp[g] < he[g] && (best < 0 || trim_after(bv, hv[g]))) { best = g; bv = hv[g]; }
        if (rank >= b) acc = __fadd_rn(acc, bv);
#pragma unroll
        for (int g = 0; g < 4; ++g)
          if (g == best) {
            col[hp[g] * W] = anydead ? fill[hp[g]] : 0.f;
            ++hp[g];
            hv[g] = col[min(hp[g], M - 1u) * W];
          }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g)                  // what the rank window left unread
        for (uint32_t j = hp[g]; j < he[g]; ++j) col[j * W] = anydead ? fill[j] : 0.f;
      const uint32_t t = win * W + mc;
      if (t < span) __builtin_nontemporal_store(__fdiv_rn(acc, a.div), a.out + base + t);
    }
    __syncthreads();
  }
}

}  // namespace fc
