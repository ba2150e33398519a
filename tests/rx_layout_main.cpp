// Prints rx_layout (csrc/rx_layout.h) for the geometries on the command line, seven numbers each:
//   S B flags de_on nsets taps pllw_bytes      (filter f has taps + f taps; the default decimations)
// One "key values..." line per field (a region: its offset and bytes), between a "geom ..." and an
// "end" line.  Built with the host compiler and the address and undefined-behaviour sanitizers by
// tests/test_rx_layout.py.
#include <cstdio>
#include <cstdlib>

#include "../real-time-software-defined-radio_amd/csrc/rx_layout.h"

using namespace rxlayout;

static void row(const char* key, const int64_t* v, int n) {
  std::printf("%s", key);
  for (int i = 0; i < n; ++i) std::printf(" %lld", (long long)v[i]);
  std::printf("\n");
}

static void regions(const char* key, const Region* r, int n) {   // "off bytes" pairs
  std::printf("%s", key);
  for (int i = 0; i < n; ++i) std::printf(" %lld %lld", (long long)r[i].off, (long long)r[i].bytes);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 8 || (argc - 1) % 7 != 0) {
    std::fprintf(stderr, "usage: %s (S B flags de_on nsets taps pllw_bytes)...\n", argv[0]);
    return 2;
  }
  for (int a = 1; a < argc; a += 7) {
    RxGeom g{};
    g.S = std::atoll(argv[a]);
    g.B = std::atoll(argv[a + 1]);
    g.rf_decim = 10; g.audio_decim = 5; g.rds_up = 19; g.rds_down = 80;
    g.flags = std::atoi(argv[a + 2]);
    g.de_on = std::atoi(argv[a + 3]) != 0;
    g.nsets = std::atoi(argv[a + 4]);
    for (int f = 0; f < SDR_RX_NFILTERS; ++f) g.taps[f] = std::atoll(argv[a + 5]) + f;   // every filter its own length
    g.pllw_bytes = std::atoll(argv[a + 6]);
    const RxLayout L = rx_layout(g);
    std::printf("geom %s %s %s %s %s %s %s\n", argv[a], argv[a + 1], argv[a + 2], argv[a + 3], argv[a + 4], argv[a + 5], argv[a + 6]);
    const int64_t sizes[] = {L.M, L.A, L.R, L.bank_len, L.ths, L.cst, L.pcs, L.pllw_bytes, L.pcm_stride, L.total, L.de_total};
    row("sizes", sizes, 11);
    row("out_n", L.out_n, SDR_RX_NOUTPUTS);
    row("out_stride", L.out_stride, SDR_RX_NOUTPUTS);
    row("zoff", L.zoff, Z_N);
    row("zlen", L.zlen, Z_N);
    for (int q = 0; q < kMaxSets; ++q) regions("out", L.out_rg[q], SDR_RX_NOUTPUTS);
    regions("reg", L.reg, NREG);
    regions("pcm", L.pcm_rg, kMaxSets);
    regions("reset", &L.reset, 1);
    regions("de_reset", &L.de_reset, 1);
    std::printf("end\n");
  }
  return 0;
}
