// launch_blocks_check.cpp -- stand-alone check of workgroup_count (lightplane_amd/csrc/lp_launch.h), the arithmetic behind every
// launcher's workgroup count.  Built with the address and undefined-behaviour sanitizers by tests/test_launch_blocks_host.py:
//
//     launch_blocks_check ITEMS PER      ->   one line "COUNT ok" or "COUNT refused"
//
// ITEMS and PER are decimal int64 values; a signed overflow anywhere in the arithmetic aborts the program (-fno-sanitize-recover).
#include <cstdio>
#include <cstdlib>

#include "../../lightplane_amd/csrc/lp_launch.h"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s ITEMS PER\n", argv[0]);
    return 2;
  }
  const int64_t items = std::strtoll(argv[1], nullptr, 10), per = std::strtoll(argv[2], nullptr, 10);
  int64_t count = -1;
  const bool ok = lp::workgroup_count(items, per, count);
  std::printf("%lld %s\n", (long long)count, ok ? "ok" : "refused");
  return 0;
}
