// ec_stream_check -- a stand-alone host program that walks recorded mixed
// token streams through rv_ec_count_stream (the counters and the shared
// edge-token gather of rav1e_amd/csrc/rv_ec.h) and compares the rates and the
// adapted CDFs with the recorded ones.  It exists to run that host code under
// the host sanitizers; it uses no device.
//
//   python tools/ec_stream_dump.py streams.bin        (from tests/golden/ref_ec_mode.npz)
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -Iinclude tools/ec_stream_check.cpp rav1e_amd/csrc/rv_ec.hip \
//       rav1e_amd/csrc/rv_runtime.hip -o ec_stream_check
//   ./ec_stream_check streams.bin
//
// File: u32 count; per stream u32 n, u32 total, n u32 tokens, total u16 initial
// CDFs, i64 rate, total u16 final CDFs, 2 x 20 u16 gathers (vert-alike, then
// horz-alike, of the 20 partition CDFs of the final table).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "rav1e_hip.h"

template <class T>
static bool rd(FILE *f, T *p, size_t n) {
  return fread(p, sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
  if (argc != 2) return fprintf(stderr, "usage: %s streams.bin\n", argv[0]), 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 2;
  uint32_t count;
  if (!rd(f, &count, 1)) return 2;
  const int total_all = rv_ec_cdf_total_all(), part = rv_ec_cdf_total();
  long tokens = 0;
  for (uint32_t s = 0; s < count; s++) {
    uint32_t n, total;
    if (!rd(f, &n, 1) || !rd(f, &total, 1) || (int)total != total_all) return 2;
    // exact-size heap blocks: a read or write past either end is reported
    std::vector<uint32_t> tok(n);
    std::vector<uint16_t> cdf(total), fin(total), g(40);
    int64_t want;
    if (!rd(f, tok.data(), n) || !rd(f, cdf.data(), total) || !rd(f, &want, 1) ||
        !rd(f, fin.data(), total) || !rd(f, g.data(), 40))
      return 2;
    std::vector<uint16_t> two(cdf), ini(cdf);
    // the whole stream, then the same in two pieces through the state
    const long rate = rv_ec_count_stream(tok.data(), n, cdf.data(), nullptr);
    uint32_t st[3] = {0x8000, (uint16_t)-9, 0};
    const long r1 = rv_ec_count_stream(tok.data(), n / 2, two.data(), st);
    const long r2 = rv_ec_count_stream(tok.data() + n / 2, n - n / 2, two.data(), st);
    if (rate != want || r1 + r2 != want || memcmp(cdf.data(), fin.data(), 2 * total) ||
        memcmp(two.data(), fin.data(), 2 * total))
      return fprintf(stderr, "stream %u: rate %ld + %ld / %ld, recorded %lld\n", s, r1, r2, rate,
                     (long long)want), 1;
    for (int k = 0; k < 2; k++)
      for (int i = 0; i < 20; i++)
        if (rv_ec_partition_gather(cdf.data() + part + 11 * i, k + 1) != g[20 * k + i])
          return fprintf(stderr, "stream %u: gather %d of partition CDF %d\n", s, k + 1, i), 1;
    // the bytes too: the encoder shares the gather and the token test
    std::vector<uint8_t> out(n / 2 + 64);
    const long nb = rv_ec_code_stream(tok.data(), n, ini.data(), out.data(), out.size());
    if (nb < 0 || memcmp(ini.data(), fin.data(), 2 * total))
      return fprintf(stderr, "stream %u: the encoder's CDFs\n", s), 1;
    tokens += n;
  }
  fclose(f);
  printf("ec_stream_check: %u streams, %ld tokens: OK\n", count, tokens);
  return 0;
}
