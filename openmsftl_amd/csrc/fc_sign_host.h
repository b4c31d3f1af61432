// fc_sign_host.h — the scaled-sign packet (FC_CODEC_SIGN, FC_FMT_SIGN): its word count, its wire
// layout and the host validator.  Plain C++17 with no HIP includes, so a host compiler takes it
// alone (tests/payload_validate_main.cc); fc_sign.hip includes it for the same layout on the device.
// What the validator shares with the other payload kinds is in fc_payload_host.h.
//
// The packet of a gradient of n elements is one float32 scale s and n sign bits, bit t % 32 of
// uint32 word[t / 32] (little-endian, the convention of mask_bits), in sign_words(n) words:
// ceil(n / 32) rounded up to a multiple of 4, so the words end on a 16-byte boundary.  Bits at and
// past n and the pad words are zero.
//
// Wire form, one contiguous little-endian byte string whose layout is a function of n alone:
//   0     fc_payload_hdr (128 bytes): magic "FCS1", version 1, uint64 total_bytes, 16 zero bytes,
//         then the canonical fc_packet_hdr: codec FC_CODEC_SIGN, format FC_FMT_SIGN, n, k =
//         n_entries = n, status OK, p = (double)s, every other field zero
//   128   uint32 word[sign_words(n)]
// The device readers follow no offset out of the payload: the only value they take from it is p.
#pragma once
#include "fc_payload_host.h"

namespace fc {

constexpr uint32_t kSignMagic = 0x31534346u;      // "FCS1" read as a little-endian uint32
constexpr PayloadKind kSignKind = {"sign wire", kSignMagic, true};

FC_HD inline uint64_t sign_words(uint64_t n) { return ((n + 31) / 32 + 3) & ~3ull; }
FC_HD inline uint64_t sign_wire_bytes(uint64_t n) { return kPayloadHdrBytes + 4 * sign_words(n); }

// Is the double with these bits the exact image of a float32 (NaNs: of a float32 NaN)?  Bit
// tests only: a conversion of an out-of-range double would be undefined.
inline bool sign_is_float32(uint64_t bits) {
  const uint64_t man = bits & 0xfffffffffffffull;
  const int ex = (int)((bits >> 52) & 0x7ff);
  if (ex == 0) return man == 0;                              // zero; a double denormal is no float
  if (ex == 0x7ff) return (man & 0x1fffffffull) == 0;        // inf, or a NaN with a float's payload
  const int e = ex - 1023;
  if (e > 127 || e < -149) return false;
  const int drop = 29 + (e < -126 ? -126 - e : 0);           // float denormals keep fewer bits
  return (man & ((1ull << drop) - 1ull)) == 0;
}

// FC_OK, or FC_ERR_ARG with the reason in err.  No read goes past len.
inline int sign_wire_validate(const void* bytes, size_t len, uint64_t n_expected, char* err,
                              size_t err_len) {
  typedef unsigned long long ull;
  // 1. the fixed header, and n (payload_open)
  fc_payload_hdr h;
  if (payload_open(kSignKind, bytes, len, n_expected, &h, err, err_len) != FC_OK) return FC_ERR_ARG;
  const unsigned char* p = static_cast<const unsigned char*>(bytes);
  // 2. the packet header
  const fc_packet_hdr& k = h.pkt;
  const uint64_t n = k.n;
  if (k.codec != FC_CODEC_SIGN) FC_BAD("sign wire: codec %u is not sign", k.codec);
  if (k.format != FC_FMT_SIGN) FC_BAD("sign wire: format %u is not sign", k.format);
  if (k.k != k.n) FC_BAD("sign wire: k = %u is not n = %u", k.k, k.n);
  if (k.n_entries != k.n) FC_BAD("sign wire: n_entries = %u is not n = %u", k.n_entries, k.n);
  if (k.status != FC_STATUS_OK) FC_BAD("sign wire: status %u is not OK", k.status);
  if (k.thresh || k.lower || k.index_bits || k.n_definite || k.n_cand || k.seed || k.offset ||
      k.chunk || k.key_mode || k.reserved[0] || k.reserved[1] || k.reserved[2])
    FC_BAD("sign wire: a header field that must be zero is not");
  const uint64_t pb = payload_p_bits(k);
  if (payload_p_negative(pb)) FC_BAD("sign wire: the scale p is negative");
  if (!sign_is_float32(pb)) FC_BAD("sign wire: the scale p is not a float32 value");
  // 3. the geometry: a function of n alone
  if (sign_wire_bytes(n) != (uint64_t)len)
    FC_BAD("sign wire: total_bytes %llu is not the size of n = %llu (%llu)", (ull)len, (ull)n,
           (ull)sign_wire_bytes(n));
  // 4. the tail bits and the pad words
  const uint64_t full = n / 32, words = sign_words(n);
  if (n % 32) {
    const uint32_t w = payload_rd<uint32_t>(p, kPayloadHdrBytes + 4 * full);
    if (w >> (n % 32)) FC_BAD("sign wire: a bit at or past n = %llu is set", (ull)n);
  }
  for (uint64_t i = (n + 31) / 32; i < words; ++i)
    if (payload_rd<uint32_t>(p, kPayloadHdrBytes + 4 * i) != 0)
      FC_BAD("sign wire: pad word %llu is not zero", (ull)i);
  return FC_OK;
}

}  // namespace fc
