// Stand-alone driver of the QSGD packet's host validator (openmsftl_amd/csrc/fc_qsgd_host.h), for a
// host compiler with -fsanitize=address,undefined (tests/test_qsgd_ef_host.py builds and runs it).
//
//   qsgd_validate_main LIST
// LIST: one "n_expected path" per line.  Each payload is read into a heap block of exactly its
// size (one byte in front keeps it off malloc's alignment: the validator may not assume any), so a
// read past `len` lands in a redzone.  Prints one verdict line per payload: "OK" or "BAD <reason>".
//
//   qsgd_validate_main --trunc LIST
// The same, but every payload is validated at EVERY length 0 .. size, each prefix in a heap block
// of exactly that length.  Prints per payload "TRUNC ok=<prefixes accepted> of=<prefixes tried>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>

#include "../openmsftl_amd/csrc/fc_qsgd_host.h"

static int verdict(const unsigned char* src, size_t len, unsigned long long n_expected, char* err,
                   size_t err_len) {
  unsigned char* block = static_cast<unsigned char*>(malloc(len + 1));
  if (len) memcpy(block + 1, src, len);
  const int rc = fc::qsgd_wire_validate(block + 1, len, n_expected, err, err_len);
  free(block);
  return rc;
}

int main(int argc, char** argv) {
  const bool trunc = argc == 3 && std::string(argv[1]) == "--trunc";
  if (argc != 2 && !trunc) {
    fprintf(stderr, "usage: %s [--trunc] LIST\n", argv[0]);
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
    char err[512] = "";
    if (trunc) {
      unsigned long long ok = 0;
      for (long len = 0; len <= size; ++len)
        ok += verdict(data, (size_t)len, n_expected, err, sizeof err) == FC_OK;
      printf("TRUNC ok=%llu of=%ld\n", ok, size + 1);
    } else {
      if (verdict(data, (size_t)size, n_expected, err, sizeof err) == FC_OK) printf("OK\n");
      else printf("BAD %s\n", err);
    }
    free(data);
  }
  return 0;
}
