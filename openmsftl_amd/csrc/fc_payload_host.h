// fc_payload_host.h — what the host validators of the three wire payload kinds share ('top' idx/val
// "FCW1", fc_wire_host.h; scaled sign "FCS1", fc_sign_host.h; QSGD "FCQ1", fc_qsgd_host.h): the
// unaligned reader, the bail-out, the 128-byte header of the kinds whose layout follows from the
// packet header alone, and the rules every kind opens with.  Plain C++17 with no HIP includes, so
// a host compiler takes it alone (tests/payload_validate_main.cc).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/fedcodec.h"

#if defined(__HIPCC__)
#define FC_HD __host__ __device__
#else
#define FC_HD
#endif

// Inside a validator (char* err, size_t err_len): the reason into err, and out.
#define FC_BAD(...)                            \
  do {                                         \
    snprintf(err, err_len, __VA_ARGS__);       \
    return FC_ERR_ARG;                         \
  } while (0)

namespace fc {

constexpr uint32_t kPayloadVersion = 1;
constexpr uint64_t kPayloadHdrBytes = 128;
static_assert(sizeof(fc_packet_hdr) == 96, "fc_packet_hdr layout");

// The first 128 bytes of a sign or QSGD payload; a 'top' payload keeps n_entries, nch and status
// where `zero` is (fc_wire_hdr).
struct fc_payload_hdr {
  uint32_t magic, version;
  uint64_t total_bytes;
  uint32_t zero[4];
  fc_packet_hdr pkt;
};
static_assert(sizeof(fc_payload_hdr) == kPayloadHdrBytes, "fc_payload_hdr layout");

// What tells the kinds apart in the rules they share.  tag: the prefix of every reason.
struct PayloadKind {
  const char* tag;
  uint32_t magic;
  bool reserved;                       // bytes 16..31 must be zero
};

template <typename T>
inline T payload_rd(const unsigned char* p, uint64_t off) {  // the bytes may sit at any address
  T v;
  memcpy(&v, p + off, sizeof v);
  return v;
}

// The rules every kind opens with: 1. the fixed header, then of 2. the packet header n alone.
// FC_OK with the header in *h, or FC_ERR_ARG with the reason in err.  No read goes past len.
inline int payload_open(const PayloadKind& kind, const void* bytes, size_t len, uint64_t n_expected,
                        fc_payload_hdr* h, char* err, size_t err_len) {
  typedef unsigned long long ull;
  const char* tag = kind.tag;
  if (bytes == nullptr) FC_BAD("%s: bytes is NULL", tag);
  if (len < kPayloadHdrBytes) FC_BAD("%s: %llu bytes are shorter than the 128-byte header", tag, (ull)len);
  *h = payload_rd<fc_payload_hdr>(static_cast<const unsigned char*>(bytes), 0);
  if (h->magic != kind.magic) FC_BAD("%s: bad magic 0x%08x", tag, h->magic);
  if (h->version != kPayloadVersion) FC_BAD("%s: unsupported version %u", tag, h->version);
  if (h->total_bytes != (uint64_t)len)
    FC_BAD("%s: total_bytes %llu but %llu bytes given", tag, (ull)h->total_bytes, (ull)len);
  if (kind.reserved && (h->zero[0] | h->zero[1] | h->zero[2] | h->zero[3]))
    FC_BAD("%s: the reserved bytes 16..31 are not zero", tag);
  const uint64_t n = h->pkt.n;
  if (n < 1) FC_BAD("%s: n = 0", tag);
  if (n_expected != 0 && n != n_expected)
    FC_BAD("%s: n = %llu but %llu expected", tag, (ull)n, (ull)n_expected);
  return FC_OK;
}

// The bits of the header's p (a scale, a norm), and whether they are a negative number: the sign
// bit set on anything but a NaN.  Bit tests only.
inline uint64_t payload_p_bits(const fc_packet_hdr& k) {
  return payload_rd<uint64_t>(reinterpret_cast<const unsigned char*>(&k.p), 0);
}
inline bool payload_p_negative(uint64_t pb) {
  const bool p_nan = ((pb >> 52) & 0x7ff) == 0x7ff && (pb & 0xfffffffffffffull) != 0;
  return (pb >> 63) != 0 && !p_nan;
}

}  // namespace fc
