// Walks dense_mb_check and the two LDS plans (sml_dense_mb_plan.h) on the host, for
// tests/test_dense_mb_plan.py, which compares the answers with ops/dense_persistent.py.
//   dense_mb_plan_walk      reads lines "w0,w1,...,wn batch own_targets" from stdin and prints two lines
//                           for each, "fp32<TAB>why<TAB>bytes" and "bf16<TAB>why<TAB>bytes": the check's
//                           answer and, where it is empty, the LDS the kernel needs (the plan plus
//                           DMB_STATIC_LDS), else -1
//   dense_mb_plan_walk -c   prints the DMB_* constants, one "NAME value" per line
// The table of a line is the one the GPU tests build: tanh layers with biases, kernel and bias of each
// layer one after the other in a flat buffer of exactly their size.
#include "sml_dense_mb_plan.h"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <vector>

int main(int argc, char** argv) {
  using namespace sml;
  if (argc > 1 && std::strcmp(argv[1], "-c") == 0) {
#define SHOW(name) std::printf(#name " %d\n", (int)name)
    SHOW(DMB_MAXLAYERS);
    SHOW(DMB_MAXW);
    SHOW(DMB_MAXBATCH);
    SHOW(DMB_NT);
    SHOW(DMB_TPT);
    SHOW(DMB_CHUNK);
    SHOW(DMB_MAXPARAMS);
    SHOW(DMB_LDS_BYTES);
    SHOW(DMB_STATIC_LDS);
    SHOW(DMB_FP32);
    SHOW(DMB_BF16);
    SHOW(DMB_TILES_BF16);
    SHOW(DMB_MAXPARAMS_BF16);
#undef SHOW
    return 0;
  }
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string ws;
    int batch = 0, own = 0;
    if (!(in >> ws >> batch >> own)) {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
    std::vector<int> widths;
    std::istringstream win(ws);
    for (std::string w; std::getline(win, w, ',');) widths.push_back(std::stoi(w));
    if (widths.empty()) {
      std::fprintf(stderr, "no widths: %s\n", line.c_str());
      return 2;
    }
    const int nl = (int)widths.size() - 1;
    std::vector<DenseMBLayer> L((size_t)(nl > 0 ? nl : 1));   // the check refuses nl > DMB_MAXLAYERS before it reads one
    int64_t off = 0;
    for (int l = 0; l < nl; ++l) {
      const int fin = widths[(size_t)l], fout = widths[(size_t)l + 1];
      L[(size_t)l] = DenseMBLayer{fin, fout, 2, 1, 0.0f, 0.0f, (int)off, (int)(off + (int64_t)fin * fout)};
      off += (int64_t)fin * fout + fout;
    }
    for (int precision : {DMB_FP32, DMB_BF16}) {
      const std::string why = dense_mb_check(L.data(), nl, widths[0], batch, off, own != 0, precision);
      long bytes = -1;
      if (why.empty())
        bytes = DMB_STATIC_LDS + (precision == DMB_BF16 ? (long)dense_mb_plan_bf16(L.data(), nl, widths[0], own != 0).lds_bytes
                                                        : 4L * dense_mb_plan(L.data(), nl, widths[0], own != 0).lds_floats);
      std::printf("%s\t%s\t%ld\n", precision == DMB_BF16 ? "bf16" : "fp32", why.c_str(), bytes);
    }
  }
  return 0;
}
