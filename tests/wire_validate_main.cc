// Stand-alone driver of the wire validator (openmsftl_amd/csrc/fc_wire_host.h), for a host
// compiler with -fsanitize=address,undefined (tests/test_wire_host.py builds and runs it).
//
//   wire_validate_main LIST
// LIST: one "n_expected path" per line.  Each payload is read into a heap block of exactly its
// size, so a read past `len` lands in a redzone.  Prints one verdict line per payload:
// "OK" or "BAD <reason>".
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <sstream>
#include <string>

#include "../openmsftl_amd/csrc/fc_wire_host.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s LIST\n", argv[0]);
    return 2;
  }
  std::ifstream list(argv[1]);
  if (!list) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
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
    // one byte in front keeps the payload off malloc's alignment: the validator may not assume any
    unsigned char* block = static_cast<unsigned char*>(malloc((size_t)size + 1));
    unsigned char* data = block + 1;
    if (size > 0 && fread(data, 1, (size_t)size, f) != (size_t)size) {
      fprintf(stderr, "short read of %s\n", path.c_str());
      return 2;
    }
    fclose(f);
    char err[512] = "";
    const int rc = fc::wire_validate(data, (size_t)size, n_expected, err, sizeof err);
    if (rc == FC_OK) printf("OK\n");
    else printf("BAD %s\n", err);
    free(block);
  }
  return 0;
}
