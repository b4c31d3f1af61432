// fc_wire.hip — the compact wire form of FC_FMT_IDXVAL packets for MI355X (gfx950): pack a batch
// of slotted packets into contiguous byte strings (fc_wire_host.h has the layout) and unpack
// such strings back into slotted packets.  grid.y is the client; the grids and every wave's
// chunk depend on n and m alone; no workgroup waits for another (three launches instead), no
// floating-point atomics, no atomics at all: two calls give the same bytes.
//
// Pack, one wave per (client, chunk), four chunks per workgroup:
//   k_wire_count    streams the chunk's listed entries (lane l: entries l + 64 r, kWR rounds of
//                   loads in flight), applies the keep rule of fc_packets_gram (gram_meta /
//                   gram_rule / gram_value over entry_kept, not restated; the quarter an entry is
//                   listed under must match its index, as there) and counts the kept entries per
//                   quarter by ballots: the chunk's new quarter-offset word goes to the workspace.
//   k_wire_scan     one 1024-thread workgroup per client: the exclusive prefix sum of the counts
//                   over the chunks, 1024 chunks per step with a carry (a DPP scan inside each
//                   wave, the sixteen wave totals through LDS), start[] to the workspace; then the
//                   verdict (the source status, the capacity) and the 128-byte header.
//   k_wire_compact  reads the entries a second time and ballot-compacts the kept ones to
//                   start[c]: the kept lanes of a round write consecutive positions (coalesced
//                   within the wave); also the table words of its chunk, and chunk 0's wave the
//                   zeroed pads.  It writes nothing when the verdict is not OK.
// A listed entry is read twice.  Every store into a wire buffer is below the capacity the scan
// kernel checked total_bytes against; entry positions are checked against E on top of that.
//
// Unpack, one wave per (client, chunk): k_wire_unpack reads start[c] and the chunk's word, clamps
// them (wire_accept, wire_clamp of fc_wire_host.h) and copies the entries to its slot.  Whatever the
// bytes hold, every read is below the byte length the host passed (the sections are laid out from
// n and E, and a packet whose E does not fit the length is unpacked as an empty packet with status
// FC_STATUS_OVERFLOW) and every write lands inside [c*8192, c*8192 + 8192) of the destination.
#include "fc_state.h"
#include "fc_wire_host.h"

namespace fc {

constexpr int kWBlock = 256;                      // pack / unpack: four waves, one chunk each
constexpr int kWWaves = kWBlock / 64;
constexpr int kWR = 4;                            // rounds (x 64 lanes) of entry loads in flight
constexpr int kWScanBlock = 1024;                 // k_wire_scan: chunks per step
constexpr int kWScanWaves = kWScanBlock / 64;
constexpr uint64_t kWSkip = ~0ull;                // verdict: nothing of this client is written

struct WireArgs {
  const fc_packet_view* views;                    // DEVICE array of m views (pack: source; unpack: destination)
  const fc_wire_job* jobs;                        // DEVICE array of m wire buffers
  uint64_t* verdict;                              // [m] E, or kWSkip
  uint64_t* word;                                 // [m][nch] quarter-offset words over the kept entries
  uint32_t* start;                                // [m][nch] exclusive prefix sum of the counts
  uint64_t n;
  uint32_t m, nch;
};

typedef __attribute__((address_space(1))) const uint64_t wu64;

// The pass both pack kernels make over chunk c of one packet: the listed entries in order, lane l
// taking entries l + 64 r, kWR rounds of loads in flight (lanes past the end re-read the last
// entry), and for every round f(kept, quarter, chunk-local index, value) in all 64 lanes.  Kept is
// fc_packets_gram's rule; the quarter an entry is listed under (from its position and the chunk's
// three inner quarter offsets) must match its index, as there.
template <typename F>
__device__ __forceinline__ void wire_for_entries(const GramMeta& meta, uint32_t c, int lane, F&& f) {
  const uint64_t base = (uint64_t)c * kChunk;
  const uint64_t qo = uni64(((wu64*)uni_ptr(meta.qoff))[c]);
  uint32_t s_, b0, b1, b2, en;
  gram_range(qo, 0, &s_, &b0);
  gram_range(qo, 1, &s_, &b1);
  gram_range(qo, 2, &s_, &b2);
  gram_range(qo, 3, &s_, &en);                     // entries [0, en) of the slot, en <= kChunk
  if (en == 0) return;                             // uniform: nothing listed here
  const GramRule r = gram_rule(meta, base);
  gu16* pidx = (gu16*)uni_ptr(meta.idx) + base;
  gf32* pval = (gf32*)uni_ptr(meta.val) + base;
  const uint32_t last = en - 1u;
  for (uint32_t e0 = 0; e0 < en; e0 += (uint32_t)(kWR * 64)) {
    uint32_t lcs[kWR];
    float vs[kWR];
#pragma unroll
    for (int rr = 0; rr < kWR; ++rr) {
      const uint32_t e = min(e0 + (uint32_t)(lane + rr * 64), last);
      lcs[rr] = pidx[e];
      vs[rr] = pval[e];
    }
#pragma unroll
    for (int rr = 0; rr < kWR; ++rr) {
      const uint32_t e = e0 + (uint32_t)(lane + rr * 64);
      const uint32_t qe = (uint32_t)(e >= b0) + (uint32_t)(e >= b1) + (uint32_t)(e >= b2);
      float x;
      const bool ok = (e < en) & gram_value(r, base, lcs[rr], vs[rr], &x) & ((lcs[rr] >> 11) == qe);
      f(ok, qe, lcs[rr], vs[rr]);
    }
  }
}

__global__ __launch_bounds__(kWBlock) void k_wire_count(WireArgs a) {
  __shared__ GramMeta meta;
  const int lane = lane_id();
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t client = blockIdx.y;
  if (threadIdx.x == 0) meta = gram_meta(a.views[client]);
  __syncthreads();
  const uint32_t c = blockIdx.x * kWWaves + w;     // uniform per wave
  if (c >= a.nch) return;
  uint32_t k1 = 0, k2 = 0, k3 = 0, k4 = 0;         // kept entries below quarter 1, 2, 3, in all
  wire_for_entries(meta, c, lane, [&](bool ok, uint32_t qe, uint32_t, float) {
    k1 += __popcll(__ballot(ok & (qe < 1u)));
    k2 += __popcll(__ballot(ok & (qe < 2u)));
    k3 += __popcll(__ballot(ok & (qe < 3u)));
    k4 += __popcll(__ballot(ok));
  });
  if (lane == 0)
    a.word[(uint64_t)client * a.nch + c] =
        (uint64_t)k1 | ((uint64_t)k2 << 16) | ((uint64_t)k3 << 32) | ((uint64_t)k4 << 48);
}

__global__ __launch_bounds__(kWScanBlock) void k_wire_scan(WireArgs a) {
  __shared__ uint32_t s_w[kWScanWaves];
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const uint32_t client = blockIdx.x;
  const uint64_t* word = a.word + (uint64_t)client * a.nch;
  uint32_t* start = a.start + (uint64_t)client * a.nch;
  uint64_t carry = 0;                              // kept entries of the chunks before this step
  for (uint32_t c0 = 0; c0 < a.nch; c0 += kWScanBlock) {
    const uint32_t c = c0 + (uint32_t)tid;
    const uint32_t cnt = c < a.nch ? (uint32_t)(word[c] >> 48) : 0u;
    const uint32_t inc = wave_incl_scan(cnt);
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < kWScanWaves; ++i) {
      const uint32_t s = s_w[i];
      if (i < w) before += s;
      tot += s;
    }
    __syncthreads();
    // a start that does not fit 32 bits belongs to a packet the verdict below refuses
    if (c < a.nch) start[c] = (uint32_t)(carry + before + inc - cnt);
    carry += tot;
  }
  if (tid != 0) return;
  // ---- the verdict and the header ----
  const fc_wire_job job = a.jobs[client];
  const fc_packet_hdr src = *a.views[client].hdr;
  const uint64_t E = carry;
  uint32_t status = src.status;
  uint64_t total = kWireHdrBytes;
  if (status == FC_STATUS_OK) {
    total = E <= 0xffffffffull ? wire_layout(a.n, E).total : ~0ull;
    if (total > job.bytes) status = FC_STATUS_OVERFLOW;
  }
  a.verdict[client] = status == FC_STATUS_OK ? E : kWSkip;
  if (job.wire == nullptr || job.bytes < kWireHdrBytes) return;
  fc_wire_hdr h;
  h.magic = kWireMagic; h.version = kWireVersion;
  h.total_bytes = total;                           // OVERFLOW: the size the packet needs
  h.n_entries = E; h.nch = a.nch; h.status = status;
  h.pkt.thresh = src.thresh; h.pkt.lower = src.thresh;
  h.pkt.n = src.n; h.pkt.k = src.k; h.pkt.n_entries = (uint32_t)E; h.pkt.index_bits = src.index_bits;
  h.pkt.codec = src.codec; h.pkt.status = FC_STATUS_OK; h.pkt.n_definite = 0; h.pkt.n_cand = 0;
  h.pkt.seed = src.seed; h.pkt.offset = src.offset; h.pkt.p = src.p;
  h.pkt.chunk = src.chunk; h.pkt.format = src.format; h.pkt.key_mode = src.key_mode;
  h.pkt.reserved[0] = h.pkt.reserved[1] = h.pkt.reserved[2] = 0;
  *reinterpret_cast<fc_wire_hdr*>(job.wire) = h;
}

__global__ __launch_bounds__(kWBlock) void k_wire_compact(WireArgs a) {
  __shared__ GramMeta meta;
  const int lane = lane_id();
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t client = blockIdx.y;
  const uint64_t E = a.verdict[client];            // uniform
  if (E == kWSkip) return;
  if (threadIdx.x == 0) meta = gram_meta(a.views[client]);
  __syncthreads();
  const uint32_t c = blockIdx.x * kWWaves + w;     // uniform per wave
  if (c >= a.nch) return;
  const WireLayout L = wire_layout(a.n, E);
  unsigned char* wire = static_cast<unsigned char*>(uni_ptr(a.jobs[client].wire));
  uint16_t* oidx = reinterpret_cast<uint16_t*>(wire + L.off_idx);
  uint32_t* oval = reinterpret_cast<uint32_t*>(wire + L.off_val);
  const uint64_t neww = a.word[(uint64_t)client * a.nch + c];
  const uint32_t st = a.start[(uint64_t)client * a.nch + c];
  if (lane == 0) {
    reinterpret_cast<uint64_t*>(wire + L.off_qoff)[c] = neww;
    reinterpret_cast<uint32_t*>(wire + L.off_start)[c] = st;
  }
  if (c == 0) {                                    // the pads: at most 15 bytes per section
    const uint64_t pad[4][2] = {{L.off_qoff + 8 * L.nch, L.off_start}, {L.off_start + 4 * L.nch, L.off_idx},
                                {L.off_idx + 2 * E, L.off_val}, {L.off_val + 4 * E, L.total}};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const uint64_t o = pad[s][0] + (uint32_t)lane;
      if (o < pad[s][1]) wire[o] = 0;
    }
  }
  uint64_t pos = st;                               // uniform: where the round's first kept entry goes
  wire_for_entries(meta, c, lane, [&](bool ok, uint32_t, uint32_t lc, float v) {
    const uint64_t mask = __ballot(ok);
    const uint64_t d = pos + prefix_count(mask);
    if (ok && d < E) {                             // d < E: inside both sections whatever was counted
      oidx[d] = (uint16_t)lc;
      oval[d] = __float_as_uint(v);                // the stored bits, -0.0 and NaN payloads included
    }
    pos += (uint32_t)__popcll(mask);
  });
}

// One wave per (client, chunk) of the destination packets.
__global__ __launch_bounds__(kWBlock) void k_wire_unpack(WireArgs a) {
  const int lane = lane_id();
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t client = blockIdx.y;
  const uint32_t c = blockIdx.x * kWWaves + w;     // uniform per wave
  if (c >= a.nch) return;
  const fc_wire_job job = a.jobs[client];
  const fc_packet_view dst = a.views[client];
  const unsigned char* wire = static_cast<const unsigned char*>(uni_ptr(job.wire));
  const uint64_t bytes = uni64(job.bytes);
  // the header: the geometry must be the caller's and the sections must fit the bytes given
  bool valid = bytes >= kWireHdrBytes;             // uniform
  uint64_t E = 0;
  uint32_t wstatus = FC_STATUS_OVERFLOW;
  if (valid) {
    const fc_wire_hdr* h = reinterpret_cast<const fc_wire_hdr*>(wire);
    E = uni64(h->n_entries);
    wstatus = uni32(h->status);
    valid = wire_accept(h, a.n, a.nch, bytes, E, [](uint32_t x) { return uni32(x); });   // uniform words
    if (!valid) E = 0;
  }
  if (c == 0 && lane < (int)(sizeof(fc_packet_hdr) / 4)) {    // the header, one 32-bit word per lane
    constexpr uint32_t kStatusWord = offsetof(fc_packet_hdr, status) / 4;
    uint32_t v;
    if (valid) {
      v = reinterpret_cast<const uint32_t*>(wire + offsetof(fc_wire_hdr, pkt))[lane];
      if ((uint32_t)lane == kStatusWord && wstatus != FC_STATUS_OK) v = wstatus;
    } else {                                       // an empty packet of length n that says why
      fc_packet_hdr o;
      memset(&o, 0, sizeof o);
      o.n = (uint32_t)a.n; o.chunk = kChunk; o.format = FC_FMT_IDXVAL; o.index_bits = 1;
      o.thresh = kSelectNothing; o.lower = kSelectNothing; o.codec = FC_CODEC_TOP;
      o.status = FC_STATUS_OVERFLOW;
      uint32_t words[sizeof(fc_packet_hdr) / 4];
      memcpy(words, &o, sizeof o);
      v = 0;
#pragma unroll
      for (uint32_t i = 0; i < sizeof(fc_packet_hdr) / 4; ++i) v = (uint32_t)lane == i ? words[i] : v;
    }
    reinterpret_cast<uint32_t*>(const_cast<fc_packet_hdr*>(dst.hdr))[lane] = v;
  }
  uint32_t q1 = 0, q2 = 0, q3 = 0, cnt = 0;
  uint64_t st = 0;
  if (valid) {
    const WireLayout L = wire_layout(a.n, E);
    const uint64_t qo = reinterpret_cast<const uint64_t*>(wire + L.off_qoff)[c];
    const WireChunk<uint64_t> k = wire_clamp(qo, reinterpret_cast<const uint32_t*>(wire + L.off_start)[c], E);
    st = k.st; cnt = k.cnt; q3 = k.q3; q2 = k.q2; q1 = k.q1;
    // entries [st, st + cnt) are below E: inside the idx and val sections, so inside `bytes`
    const uint16_t* sidx = reinterpret_cast<const uint16_t*>(wire + L.off_idx) + st;
    const uint32_t* sval = reinterpret_cast<const uint32_t*>(wire + L.off_val) + st;
    uint16_t* didx = const_cast<uint16_t*>(static_cast<const uint16_t*>(dst.idx)) + (uint64_t)c * kChunk;
    uint32_t* dval = reinterpret_cast<uint32_t*>(const_cast<float*>(dst.val)) + (uint64_t)c * kChunk;
    for (uint32_t e0 = 0; e0 < cnt; e0 += (uint32_t)(kWR * 64)) {
      uint16_t li[kWR];
      uint32_t lv[kWR];
#pragma unroll
      for (int rr = 0; rr < kWR; ++rr) {
        const uint32_t e = min(e0 + (uint32_t)(lane + rr * 64), cnt - 1u);
        li[rr] = sidx[e];
        lv[rr] = sval[e];
      }
#pragma unroll
      for (int rr = 0; rr < kWR; ++rr) {
        const uint32_t e = e0 + (uint32_t)(lane + rr * 64);
        if (e < cnt) {                             // cnt <= kChunk: inside the chunk's slot
          didx[e] = li[rr];
          dval[e] = lv[rr];
        }
      }
    }
  }
  if (lane == 0) {
    const_cast<uint32_t*>(dst.cnt)[c] = cnt;
    const_cast<uint64_t*>(dst.qoff)[c] =
        (uint64_t)q1 | ((uint64_t)q2 << 16) | ((uint64_t)q3 << 32) | ((uint64_t)cnt << 48);
  }
}

}  // namespace fc

// ---- C ABI ---------------------------------------------------------------------------------
namespace {
struct WireGeom { uint32_t nch; size_t verdict_bytes, word_bytes, bytes; };
WireGeom wire_geom(uint64_t n, int m) {
  WireGeom g;
  g.nch = num_chunks(n);
  g.verdict_bytes = ((size_t)m * 8 + 255) & ~(size_t)255;
  g.word_bytes = (((size_t)m * g.nch * 8) + 255) & ~(size_t)255;
  g.bytes = g.verdict_bytes + g.word_bytes + ((((size_t)m * g.nch * 4) + 255) & ~(size_t)255);
  return g;
}
}  // namespace

extern "C" {

uint64_t fc_wire_bytes(uint64_t n, uint64_t n_entries) {
  if (n == 0 || n > 0xffffffffull || n_entries > 0xffffffffull) return 0;
  return fc::wire_layout(n, n_entries).total;
}

size_t fc_wire_workspace_bytes(uint64_t n, int m) {
  if (n == 0 || n > 0xffffffffull || m < 1 || m > 65535) return 0;
  return wire_geom(n, m).bytes;
}

int fc_wire_validate(const void* host_bytes, size_t len, uint64_t n_expected) {
  return fc::wire_validate(host_bytes, len, n_expected, g_err, sizeof g_err);
}

int fc_wire_pack_batch(const fc_packet_view* views_dev, const fc_wire_job* jobs_dev, int m, uint64_t n,
                       void* ws, size_t ws_bytes, fc_stream_t stream) {
  FC_CHECK(views_dev != nullptr, "views_dev is NULL");
  FC_CHECK(jobs_dev != nullptr, "jobs_dev is NULL");
  FC_CHECK(ws != nullptr, "workspace is NULL");
  FC_CHECK(m >= 1 && m <= 65535, "m=%d outside [1, 65535]", m);
  FC_CHECK(n >= 1 && n <= 0xffffffffull, "n=%llu outside [1, 2^32-1]", (unsigned long long)n);
  FC_CHECK(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
  const WireGeom g = wire_geom(n, m);
  if (ws_bytes < g.bytes)
    return fail(FC_ERR_WORKSPACE, "workspace %zu B < %zu B needed", ws_bytes, g.bytes);
  WireArgs a;
  memset(&a, 0, sizeof a);
  a.views = views_dev; a.jobs = jobs_dev; a.n = n; a.m = (uint32_t)m; a.nch = g.nch;
  a.verdict = reinterpret_cast<uint64_t*>(ws);
  a.word = reinterpret_cast<uint64_t*>(static_cast<char*>(ws) + g.verdict_bytes);
  a.start = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + g.verdict_bytes + g.word_bytes);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((g.nch + kWWaves - 1) / kWWaves, (uint32_t)m);
  hipLaunchKernelGGL(k_wire_count, grid, dim3(kWBlock), 0, s, a);
  FC_LAUNCHED("k_wire_count");
  hipLaunchKernelGGL(k_wire_scan, dim3((uint32_t)m), dim3(kWScanBlock), 0, s, a);
  FC_LAUNCHED("k_wire_scan");
  hipLaunchKernelGGL(k_wire_compact, grid, dim3(kWBlock), 0, s, a);
  FC_LAUNCHED("k_wire_compact");
  return FC_OK;
}

int fc_wire_unpack_batch(const fc_wire_job* jobs_dev, const fc_packet_view* views_dev, int m, uint64_t n,
                         fc_stream_t stream) {
  FC_CHECK(jobs_dev != nullptr, "jobs_dev is NULL");
  FC_CHECK(views_dev != nullptr, "views_dev is NULL");
  FC_CHECK(m >= 1 && m <= 65535, "m=%d outside [1, 65535]", m);
  FC_CHECK(n >= 1 && n <= 0xffffffffull, "n=%llu outside [1, 2^32-1]", (unsigned long long)n);
  WireArgs a;
  memset(&a, 0, sizeof a);
  a.views = views_dev; a.jobs = jobs_dev; a.n = n; a.m = (uint32_t)m; a.nch = num_chunks(n);
  const dim3 grid((a.nch + kWWaves - 1) / kWWaves, (uint32_t)m);
  hipLaunchKernelGGL(k_wire_unpack, grid, dim3(kWBlock), 0, (hipStream_t)stream, a);
  FC_LAUNCHED("k_wire_unpack");
  return FC_OK;
}

}  // extern "C"
