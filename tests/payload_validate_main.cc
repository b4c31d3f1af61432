// Stand-alone driver of the host-side rules of the three wire payload kinds
// (openmsftl_amd/csrc/fc_wire_host.h, fc_sign_host.h, fc_qsgd_host.h over fc_payload_host.h), for a
// host compiler with -fsanitize=address,undefined (tests/payload_standalone.py builds and runs it).
// KIND is wire, sign or qsgd.
//
//   payload_validate_main KIND LIST
// LIST: one "n_expected path" per line.  Each payload is validated in a heap block of exactly its
// size (one byte in front keeps it off malloc's alignment: the validator may not assume any), so a
// read past `len` lands in a redzone.  Prints one verdict line per payload: "OK" or "BAD <reason>".
//
//   payload_validate_main KIND --trunc LIST
// The same, but every payload is validated at EVERY length 0 .. size, each prefix in a heap block
// of exactly that length.  Prints per payload "TRUNC ok=<prefixes accepted> of=<prefixes tried>".
//
//   payload_validate_main wire --clamp LIST
// LIST: one "n path" per line, n the length the reader expects.  The payload, in a heap block of
// exactly its size and of the block's own alignment (as a device buffer has it), goes through what
// the device readers (k_wire_unpack, the wire fold) do with bytes nobody validated: wire_accept,
// then for every chunk wire_clamp and a read of every idx and val entry of [st, st + cnt) through
// the section offsets.  Prints "REJECT", or "ACCEPT E=<entries> exact=<1 if every chunk's clamp
// returned the stored words, else 0>"; exits with 1 if a clamped range leaves [0, E) or its
// boundaries are out of order.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>

#include "../openmsftl_amd/csrc/fc_qsgd_host.h"
#include "../openmsftl_amd/csrc/fc_sign_host.h"
#include "../openmsftl_amd/csrc/fc_wire_host.h"

typedef int (*validate_fn)(const void*, size_t, uint64_t, char*, size_t);

static volatile unsigned long long g_sink;

// The readers' path over one buffer; false: a range left [0, E).
static bool clamp_walk(const unsigned char* data, size_t size, unsigned long long n) {
  const uint32_t nch = (uint32_t)((n + fc::kWireChunk - 1) / fc::kWireChunk);
  if (size < fc::kWireHdrBytes) {                   // the header is not read at all
    printf("REJECT\n");
    return true;
  }
  const fc::fc_wire_hdr* h = reinterpret_cast<const fc::fc_wire_hdr*>(data);
  const uint64_t E = h->n_entries;
  if (!fc::wire_accept(h, n, nch, size, E, [](uint32_t x) { return x; })) {
    printf("REJECT\n");
    return true;
  }
  const fc::WireLayout L = fc::wire_layout(n, E);
  const uint64_t* qoff = reinterpret_cast<const uint64_t*>(data + L.off_qoff);
  const uint32_t* start = reinterpret_cast<const uint32_t*>(data + L.off_start);
  const uint16_t* idx = reinterpret_cast<const uint16_t*>(data + L.off_idx);
  const uint32_t* val = reinterpret_cast<const uint32_t*>(data + L.off_val);
  bool exact = true;
  unsigned long long sum = 0;                       // keeps the entry reads alive
  for (uint32_t c = 0; c < nch; ++c) {
    const uint64_t qo = qoff[c];
    const uint32_t st0 = start[c];
    // both widths the readers use must agree
    const fc::WireChunk<uint32_t> k = fc::wire_clamp<uint32_t>(qo, st0, (uint32_t)E);
    const fc::WireChunk<uint64_t> k64 = fc::wire_clamp<uint64_t>(qo, st0, E);
    if (k64.st != k.st || k64.cnt != k.cnt || k64.q1 != k.q1 || k64.q2 != k.q2 || k64.q3 != k.q3) {
      fprintf(stderr, "chunk %u: the 32-bit and 64-bit clamps differ\n", c);
      return false;
    }
    if (!(k.q1 <= k.q2 && k.q2 <= k.q3 && k.q3 <= k.cnt && k.cnt <= FC_CHUNK && k.st <= E &&
          (uint64_t)k.st + k.cnt <= E)) {
      fprintf(stderr, "chunk %u: st %u q %u %u %u cnt %u leaves [0, %llu)\n", c, k.st, k.q1, k.q2, k.q3,
              k.cnt, (unsigned long long)E);
      return false;
    }
    exact = exact && k.st == st0 &&
            qo == ((uint64_t)k.q1 | ((uint64_t)k.q2 << 16) | ((uint64_t)k.q3 << 32) | ((uint64_t)k.cnt << 48));
    for (uint32_t e = k.st; e < k.st + k.cnt; ++e) sum += idx[e] + (unsigned long long)val[e];
  }
  g_sink = sum;
  printf("ACCEPT E=%llu exact=%d\n", (unsigned long long)E, exact ? 1 : 0);
  return true;
}

// `front` bytes before the payload in a heap block that ends where the payload ends
static unsigned char* block_of(const unsigned char* src, size_t len, size_t front) {
  unsigned char* block = static_cast<unsigned char*>(malloc(len + front));
  if (len) memcpy(block + front, src, len);
  return block;
}

int main(int argc, char** argv) {
  const std::string kind = argc > 1 ? argv[1] : "", mode = argc == 4 ? argv[2] : "";
  const validate_fn validate = kind == "wire" ? fc::wire_validate
                               : kind == "sign" ? fc::sign_wire_validate
                               : kind == "qsgd" ? fc::qsgd_wire_validate : nullptr;
  const bool trunc = mode == "--trunc", clamp = mode == "--clamp" && kind == "wire";
  if (!validate || (argc != 3 && !trunc && !clamp)) {
    fprintf(stderr, "usage: %s wire|sign|qsgd [--trunc] LIST, or %s wire --clamp LIST\n", argv[0], argv[0]);
    return 2;
  }
  std::ifstream list(argv[argc - 1]);
  if (!list) {
    fprintf(stderr, "cannot open %s\n", argv[argc - 1]);
    return 2;
  }
  std::string line;
  while (std::getline(list, line)) {
    if (line.empty()) continue;
    std::istringstream is(line);
    unsigned long long n_expected = 0;
    std::string path;
    is >> n_expected;
    std::getline(is >> std::ws, path);
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) {
      fprintf(stderr, "cannot open %s\n", path.c_str());
      return 2;
    }
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char* data = static_cast<unsigned char*>(malloc((size_t)size + 1));
    if (size > 0 && fread(data, 1, (size_t)size, f) != (size_t)size) {
      fprintf(stderr, "short read of %s\n", path.c_str());
      return 2;
    }
    fclose(f);
    if (clamp) {
      unsigned char* block = block_of(data, (size_t)size, 0);
      const bool inside = clamp_walk(block, (size_t)size, n_expected);
      free(block);
      if (!inside) return 1;
    } else {
      char err[512] = "";
      unsigned long long ok = 0;
      for (long len = trunc ? 0 : size; len <= size; ++len) {
        unsigned char* block = block_of(data, (size_t)len, 1);
        ok += validate(block + 1, (size_t)len, n_expected, err, sizeof err) == FC_OK;
        free(block);
      }
      if (trunc) printf("TRUNC ok=%llu of=%ld\n", ok, size + 1);
      else if (ok) printf("OK\n");
      else printf("BAD %s\n", err);
    }
    free(data);
  }
  return 0;
}
