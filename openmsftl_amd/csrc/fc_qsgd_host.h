// fc_qsgd_host.h — the QSGD packet (FC_CODEC_QSGD, FC_FMT_QSGD): its code width and word count, its
// wire layout and the host validator.  Plain C++17 with no HIP includes, so a host compiler takes
// it alone (tests/payload_validate_main.cc); fc_qsgd.hip includes it for the same layout on the
// device.  What the validator shares with the other payload kinds is in fc_payload_host.h.
//
// The packet of a gradient of n elements at `bits` (1..14) is the float64 norm in the header's p
// and one W-bit code per element, W = 4 / 8 / 16 for bits <= 2 / 6 / 14: the sign in the code's top
// bit, the level 0..s = 2^bits in the W - 1 bits below it, packed little-endian in groups of 8
// elements (qsgd_code_words(n, bits) uint32).  Codes at and past n inside the last group are zero.
//
// Wire form, one contiguous little-endian byte string whose layout is a function of n and bits:
//   0     fc_payload_hdr (128 bytes): magic "FCQ1", version 1, uint64 total_bytes, 16 zero bytes,
//         then the canonical fc_packet_hdr: codec FC_CODEC_QSGD, format FC_FMT_QSGD, n, k = bits,
//         n_entries = n, status OK, key_mode FC_KEY_PHILOX, seed and offset (any), p = the norm,
//         every other field zero
//   128   uint32 code word[qsgd_wire_words(n, bits)]: the code words, then zero words up to a
//         multiple of 4
// The device readers follow no offset out of the payload: they take p and k from the header and
// index the codes by element; a level above s could only come from a forged payload.
#pragma once
#include "fc_payload_host.h"

namespace fc {

constexpr uint32_t kQsgdMagic = 0x31514346u;      // "FCQ1" read as a little-endian uint32
constexpr PayloadKind kQsgdKind = {"qsgd wire", kQsgdMagic, true};

FC_HD inline int qsgd_width(int bits) { return bits <= 2 ? 4 : bits <= 6 ? 8 : 16; }
// 0 for bits outside [1, 14]
FC_HD inline uint64_t qsgd_code_words(uint64_t n, int bits) {
  if (bits < 1 || bits > 14) return 0;
  return (n + 7) / 8 * (uint64_t)(qsgd_width(bits) / 4);
}
FC_HD inline uint64_t qsgd_wire_words(uint64_t n, int bits) {
  return (qsgd_code_words(n, bits) + 3) & ~3ull;
}
FC_HD inline uint64_t qsgd_wire_bytes(uint64_t n, int bits) {
  if (bits < 1 || bits > 14) return 0;
  return kPayloadHdrBytes + 4 * qsgd_wire_words(n, bits);
}

// FC_OK, or FC_ERR_ARG with the reason in err.  No read goes past len.
inline int qsgd_wire_validate(const void* bytes, size_t len, uint64_t n_expected, char* err,
                              size_t err_len) {
  typedef unsigned long long ull;
  // 1. the fixed header, and n (payload_open)
  fc_payload_hdr h;
  if (payload_open(kQsgdKind, bytes, len, n_expected, &h, err, err_len) != FC_OK) return FC_ERR_ARG;
  const unsigned char* p = static_cast<const unsigned char*>(bytes);
  // 2. the packet header
  const fc_packet_hdr& k = h.pkt;
  const uint64_t n = k.n;
  if (k.codec != FC_CODEC_QSGD) FC_BAD("qsgd wire: codec %u is not qsgd", k.codec);
  if (k.format != FC_FMT_QSGD) FC_BAD("qsgd wire: format %u is not qsgd", k.format);
  if (k.k < 1 || k.k > 14) FC_BAD("qsgd wire: k = %u bits outside [1, 14]", k.k);
  if (k.n_entries != k.n) FC_BAD("qsgd wire: n_entries = %u is not n = %u", k.n_entries, k.n);
  if (k.status != FC_STATUS_OK) FC_BAD("qsgd wire: status %u is not OK", k.status);
  if (k.key_mode != FC_KEY_PHILOX) FC_BAD("qsgd wire: key_mode %u is not philox", k.key_mode);
  if (k.thresh || k.lower || k.index_bits || k.n_definite || k.n_cand || k.chunk || k.reserved[0] ||
      k.reserved[1] || k.reserved[2])
    FC_BAD("qsgd wire: a header field that must be zero is not");
  if (payload_p_negative(payload_p_bits(k))) FC_BAD("qsgd wire: the norm p is negative");
  // 3. the geometry: a function of n and bits alone
  const int bits = (int)k.k;
  if (qsgd_wire_bytes(n, bits) != (uint64_t)len)
    FC_BAD("qsgd wire: total_bytes %llu is not the size of n = %llu at %d bits (%llu)", (ull)len,
           (ull)n, bits, (ull)qsgd_wire_bytes(n, bits));
  // 4. the codes: no level above s, nothing at or past n, zero pad words
  const uint32_t W = (uint32_t)qsgd_width(bits), per = 32 / W;
  const uint32_t lmask = (1u << (W - 1)) - 1u, s = 1u << bits;
  const uint64_t words = qsgd_code_words(n, bits), full = n / per;        // words wholly below n
  // Two words at a time first: s is a power of two, so a level exceeds it when a bit above bit
  // `bits` is set, or bit `bits` and any bit below it.  In every W-bit field at once: `low +
  // lows` carries into bit `bits` exactly where the low bits are not all zero, and cannot leave
  // the field's W - 1 level bits (bits + 1 <= W - 1).  (With one test per code an aggregate_wire
  // round of 32 x 25.5 M 2-bit payloads took 306 ms, nearly all of it here; this loop takes
  // 2.4 ms per 12.7 MB payload.)  The first pair that fails is walked code by code below for the
  // message.
  uint64_t one = 1, rep = 0;
  for (uint32_t j = 0; j < 64 / W; ++j) rep |= one << (j * W);
  const uint64_t tops = rep << bits, lows = tops - rep, highs = (rep << (W - 1)) - (tops << 1);
  uint64_t first = 0;
  for (; first + 2 <= full; first += 2) {
    const uint64_t w = payload_rd<uint64_t>(p, kPayloadHdrBytes + 4 * first);
    if ((w & highs) | ((((w & lows) + lows) & w) & tops)) break;
  }
  for (uint64_t i = first; i < full; ++i) {
    const uint32_t w = payload_rd<uint32_t>(p, kPayloadHdrBytes + 4 * i);
    for (uint32_t j = 0; j < per; ++j)
      if (((w >> (j * W)) & lmask) > s)
        FC_BAD("qsgd wire: the code of element %llu has level %u above s = %u", (ull)(i * per + j),
               (w >> (j * W)) & lmask, s);
  }
  if (n % per) {
    const uint32_t w = payload_rd<uint32_t>(p, kPayloadHdrBytes + 4 * full), live = (uint32_t)(n % per);
    for (uint32_t j = 0; j < live; ++j)
      if (((w >> (j * W)) & lmask) > s)
        FC_BAD("qsgd wire: the code of element %llu has level %u above s = %u", (ull)(full * per + j),
               (w >> (j * W)) & lmask, s);
    if (w >> (live * W)) FC_BAD("qsgd wire: a code at or past n = %llu is not zero", (ull)n);
  }
  for (uint64_t i = (n + per - 1) / per; i < words; ++i)
    if (payload_rd<uint32_t>(p, kPayloadHdrBytes + 4 * i) != 0)
      FC_BAD("qsgd wire: a code at or past n = %llu is not zero", (ull)n);
  for (uint64_t i = words; i < qsgd_wire_words(n, bits); ++i)
    if (payload_rd<uint32_t>(p, kPayloadHdrBytes + 4 * i) != 0)
      FC_BAD("qsgd wire: pad word %llu is not zero", (ull)i);
  return FC_OK;
}

}  // namespace fc
