// Asks the bf16 per-event Dense scorer's check and plan (sml_dense_serve_bf16.h) on the host, for
// tests/test_dense_serve_bf16_limits.py, which compares the answers with ops/serve.py
// DenseScoringServer.supports / kernel_for(precision="bf16").
//   dense_serve_bf16_check       reads lines "w0,w1,...,wn" from stdin and prints one line for each,
//                                "why<TAB>img_words<TAB>bf16-lds|bf16-stream<TAB>lds_bytes": the check's
//                                answer, the words of the image, where the plan puts it and the plan's
//                                dynamic LDS bytes
//   dense_serve_bf16_check -c    prints the DSVB_* constants, one "NAME value" per line
// The table of a line is the one ops/dense_forward_wide.py image_table builds, with tanh layers.
#include "sml_dense_serve_bf16.h"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

int main(int argc, char** argv) {
  using namespace sml;
  if (argc > 1 && std::strcmp(argv[1], "-c") == 0) {
#define SHOW(name) std::printf(#name " %d\n", (int)name)
    SHOW(DSVB_MAXD);
    SHOW(DSVB_EB);
    SHOW(DSVB_NT);
    SHOW(DSVB_STATIC_LDS);
    SHOW(DSVB_ACT_BYTES_MAX);
    SHOW(DSVB_LDS_IMAGE_BYTES);
#undef SHOW
    return 0;
  }
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::vector<int> widths;
    std::istringstream win(line);
    for (std::string w; std::getline(win, w, ',');) widths.push_back(std::stoi(w));
    if (widths.empty()) {
      std::fprintf(stderr, "no widths: %s\n", line.c_str());
      return 2;
    }
    const int nl = (int)widths.size() - 1;
    // at least one entry: the check refuses nl outside 1..8 before it reads one
    std::vector<DenseFwdLayer> L((size_t)(nl > 0 ? nl : 1), DenseFwdLayer{});
    for (int l = 0; l < nl; ++l) L[(size_t)l] = DenseFwdLayer{widths[(size_t)l], widths[(size_t)l + 1], 2, 0, 0};
    const bool sized = nl >= 1 && nl <= DFWW_MAXLAYERS;
    const int words = sized ? dense_fwdw_image_offsets(L.data(), nl) : 0;
    const std::string why = dense_serve_bf16_check(L.data(), nl, widths[0], sized ? words : -1);
    const DenseServeBf16Plan P = sized ? dense_serve_bf16_plan(L.data(), nl) : DenseServeBf16Plan{};
    std::printf("%s\t%d\t%s\t%d\n", why.c_str(), words, P.in_lds ? "bf16-lds" : "bf16-stream", P.lds_bytes);
  }
  return 0;
}
