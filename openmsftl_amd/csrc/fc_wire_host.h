// fc_wire_host.h — the wire format of an FC_FMT_IDXVAL packet: layout, size, the host validator
// and the two rules of the device readers that take unvalidated bytes (wire_accept, wire_clamp).
// Plain C++17 with no HIP includes, so a host compiler takes it alone
// (tests/payload_validate_main.cc); fc_wire.hip includes it for the same layout and rules on the
// device.  What the validator shares with the other payload kinds is in fc_payload_host.h.
//
// One packet is one contiguous little-endian byte string; every section starts 16-B aligned and
// pad bytes are zero:
//   0     fc_wire_hdr (128 bytes): magic "FCW1", version, total_bytes, n_entries (E), nch, status,
//         fc_packet_hdr pkt
//   128   uint64 qoff[nch]   the slotted word format over the KEPT entries: quarter 1/2/3 starts
//                            in bits 0-15 / 16-31 / 32-47, cnt in bits 48-63
//         uint32 start[nch]  exclusive prefix sum of the counts
//         uint16 idx[E]      chunk-local, ascending inside each chunk
//         float  val[E]      raw stored values (the decoders apply 1/p from pkt.p)
#pragma once
#include "fc_payload_host.h"

namespace fc {

constexpr uint32_t kWireMagic = 0x31574346u;      // "FCW1" read as a little-endian uint32
constexpr uint32_t kWireVersion = kPayloadVersion;
constexpr uint64_t kWireHdrBytes = kPayloadHdrBytes;
constexpr PayloadKind kWireKind = {"wire", kWireMagic, false};  // bytes 16..31: n_entries, nch, status
constexpr uint64_t kWireChunk = FC_CHUNK;

struct fc_wire_hdr {
  uint32_t magic, version;
  uint64_t total_bytes;
  uint64_t n_entries;
  uint32_t nch, status;
  fc_packet_hdr pkt;
};
static_assert(sizeof(fc_wire_hdr) == 128, "fc_wire_hdr layout");

struct WireLayout {
  uint64_t nch, off_qoff, off_start, off_idx, off_val, total;
};

FC_HD inline uint64_t wire_pad16(uint64_t x) { return (x + 15ull) & ~15ull; }

// Section offsets and the exact size of a packet of length n with E kept entries
// (n < 2^32 and E < 2^33: nothing overflows).
FC_HD inline WireLayout wire_layout(uint64_t n, uint64_t E) {
  WireLayout L;
  L.nch = (n + kWireChunk - 1) / kWireChunk;
  L.off_qoff = kWireHdrBytes;
  L.off_start = L.off_qoff + wire_pad16(8 * L.nch);
  L.off_idx = L.off_start + wire_pad16(4 * L.nch);
  L.off_val = L.off_idx + wire_pad16(2 * E);
  L.total = L.off_val + wire_pad16(4 * E);
  return L;
}

// ---- what a device reader (k_wire_unpack, the wire fold) does with bytes nobody validated ----
// Is the buffer behind header h (bytes >= 128: the caller checks that first) a packet of the
// caller's n and nch inside `bytes`?  E is h->n_entries as the caller read it, once.  Accepted:
// both tables and entries [0, E) of idx and val lie below `bytes`.  u is applied to every header
// word as it is read (k_wire_unpack makes them wave-uniform); no other word is read.
template <typename U>
FC_HD inline bool wire_accept(const fc_wire_hdr* h, uint64_t n, uint32_t nch, uint64_t bytes,
                                   uint64_t E, U u) {
  return u(h->magic) == kWireMagic && u(h->version) == kWireVersion && u(h->nch) == nch &&
         (uint64_t)u(h->pkt.n) == n && E <= 0xffffffffull && wire_layout(n, E).total <= bytes;
}

// Chunk c's entries [st, st + cnt) and its quarter boundaries 0 <= q1 <= q2 <= q3 <= cnt from the
// chunk's offsets word and start word, clamped: st + cnt <= E and cnt <= 8192 whatever the words
// hold; a payload wire_validate accepts comes back as stored.  T: the width E (< 2^32) is held in.
template <typename T>
struct WireChunk {
  T st;
  uint32_t q1, q2, q3, cnt;
};
template <typename T>
FC_HD inline T wire_min(T a, T b) { return a < b ? a : b; }
template <typename T>
FC_HD inline WireChunk<T> wire_clamp(uint64_t qo, uint32_t start, T E) {
  WireChunk<T> k;
  k.st = wire_min<T>(start, E);
  k.cnt = (uint32_t)wire_min<T>(wire_min<uint32_t>((uint32_t)(qo >> 48), (uint32_t)kWireChunk), E - k.st);
  k.q3 = wire_min<uint32_t>((uint32_t)(qo >> 32) & 0xffffu, k.cnt);
  k.q2 = wire_min<uint32_t>((uint32_t)(qo >> 16) & 0xffffu, k.q3);
  k.q1 = wire_min<uint32_t>((uint32_t)qo & 0xffffu, k.q2);
  return k;
}

inline uint32_t wire_index_bits(uint64_t n) {
  uint32_t b = 0;
  while (b < 63 && (1ull << b) < n) ++b;
  return b < 1 ? 1 : b;
}

// FC_OK, or FC_ERR_ARG with the reason in err.  No read goes past len.
inline int wire_validate(const void* bytes, size_t len, uint64_t n_expected, char* err,
                         size_t err_len) {
  typedef unsigned long long ull;
  // 1. the fixed header, and n (payload_open)
  fc_payload_hdr open;
  if (payload_open(kWireKind, bytes, len, n_expected, &open, err, err_len) != FC_OK) return FC_ERR_ARG;
  const unsigned char* p = static_cast<const unsigned char*>(bytes);
  const fc_wire_hdr h = payload_rd<fc_wire_hdr>(p, 0);
  // 2. the packet header
  const fc_packet_hdr& k = h.pkt;
  const uint64_t n = k.n;
  if (k.k > k.n) FC_BAD("wire: k = %u above n = %u", k.k, k.n);
  if (k.index_bits != wire_index_bits(n))
    FC_BAD("wire: index_bits %u, %u for n = %llu", k.index_bits, wire_index_bits(n), (ull)n);
  if (k.chunk != FC_CHUNK) FC_BAD("wire: chunk %u is not %d", k.chunk, FC_CHUNK);
  if (k.format != FC_FMT_IDXVAL) FC_BAD("wire: format %u is not idx/val", k.format);
  if (k.codec < FC_CODEC_TOP || k.codec > FC_CODEC_DROPOUT_UNBIASED)
    FC_BAD("wire: codec %u outside 1..4", k.codec);
  if (k.key_mode > FC_KEY_PHILOX) FC_BAD("wire: key_mode %u outside 0..1", k.key_mode);
  if (h.status != FC_STATUS_OK || k.status != FC_STATUS_OK)
    FC_BAD("wire: status %u / %u is not OK", h.status, k.status);
  // 3. the geometry
  const uint64_t E = h.n_entries;
  if (h.nch != (n + kWireChunk - 1) / kWireChunk)
    FC_BAD("wire: nch %u, %llu chunks for n = %llu", h.nch, (ull)((n + kWireChunk - 1) / kWireChunk), (ull)n);
  if (E > (uint64_t)len || wire_layout(n, E).total != (uint64_t)len)
    FC_BAD("wire: total_bytes %llu is not the size of n = %llu with %llu entries", (ull)len, (ull)n, (ull)E);
  const WireLayout L = wire_layout(n, E);
  // 4. the chunk table
  uint64_t run = 0;
  for (uint64_t c = 0; c < L.nch; ++c) {
    const uint64_t w = payload_rd<uint64_t>(p, L.off_qoff + 8 * c);
    const uint32_t q1 = (uint32_t)(w & 0xffffu), q2 = (uint32_t)((w >> 16) & 0xffffu),
                   q3 = (uint32_t)((w >> 32) & 0xffffu), cnt = (uint32_t)(w >> 48);
    if (!(q1 <= q2 && q2 <= q3 && q3 <= cnt && cnt <= FC_CHUNK))
      FC_BAD("wire: chunk %llu: quarter offsets %u, %u, %u, count %u out of order or above 8192",
             (ull)c, q1, q2, q3, cnt);
    const uint32_t st = payload_rd<uint32_t>(p, L.off_start + 4 * c);
    if ((uint64_t)st != run)
      FC_BAD("wire: chunk %llu: start %u is not the prefix sum %llu", (ull)c, st, (ull)run);
    run += cnt;
  }
  if (run != E || (uint64_t)k.n_entries != E)
    FC_BAD("wire: the counts sum to %llu, n_entries %llu, pkt.n_entries %u", (ull)run, (ull)E, k.n_entries);
  // 5. the indices, quarter by quarter (run <= E: every read is inside the idx section)
  run = 0;
  for (uint64_t c = 0; c < L.nch; ++c) {
    const uint64_t w = payload_rd<uint64_t>(p, L.off_qoff + 8 * c);
    const uint32_t b[5] = {0u, (uint32_t)(w & 0xffffu), (uint32_t)((w >> 16) & 0xffffu),
                           (uint32_t)((w >> 32) & 0xffffu), (uint32_t)(w >> 48)};
    for (uint32_t q = 0; q < 4; ++q) {
      int64_t prev = -1;
      for (uint32_t e = b[q]; e < b[q + 1]; ++e) {
        const uint32_t lc = payload_rd<uint16_t>(p, L.off_idx + 2 * (run + e));
        if ((int64_t)lc <= prev)
          FC_BAD("wire: chunk %llu entry %u: index %u does not ascend", (ull)c, e, lc);
        if ((lc >> 11) != q)
          FC_BAD("wire: chunk %llu entry %u: index %u is not in quarter %u", (ull)c, e, lc, q);
        if (c * kWireChunk + lc >= n)
          FC_BAD("wire: chunk %llu entry %u: element %llu is past n = %llu", (ull)c, e,
                 (ull)(c * kWireChunk + lc), (ull)n);
        prev = (int64_t)lc;
      }
    }
    run += b[4];
  }
  // 6. the pads
  const uint64_t pad[4][2] = {{L.off_qoff + 8 * L.nch, L.off_start}, {L.off_start + 4 * L.nch, L.off_idx},
                              {L.off_idx + 2 * E, L.off_val}, {L.off_val + 4 * E, L.total}};
  for (int s = 0; s < 4; ++s)
    for (uint64_t o = pad[s][0]; o < pad[s][1]; ++o)
      if (p[o] != 0) FC_BAD("wire: pad byte at offset %llu is not zero", (ull)o);
  return FC_OK;
}

}  // namespace fc
