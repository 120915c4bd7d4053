// Asks the fused Dense forwards' checks and plans (sml_dense_fwd_plan.h, sml_dense_fwdw_plan.h,
// sml_dense_fleet_fwd.h) on the host, for tests/test_dense_forward_check.py, which compares the answers
// with the Python mirrors ops/dense_forward.py, ops/dense_forward_wide.py and ops/dense_fleet_forward.py.
//   dense_fwd_check MODE                          reads cases from stdin, one per line
//   dense_fwd_check MODE WIDTHS ACTS [SCORE [N]]  one case from the command line
// MODE is narrow, wide or fleet.  A case is "w0,w1,...,wn a1,...,an score n": the widths (input first), the
// layers' activation codes (-1: a name the kernels do not know), 1 for scores against the input row, and
// the rows of a tile (wide: 64 or 128) or the models of the fleet (fleet); score and n default to 0 / 64 / 1.
// The table's offsets are the packed layout's and the image is checked at its packed size.  Prints, tab
// separated, the check's reason (empty: the kernel takes the stack), the image's floats / words and the
// plan of a stack of 1 .. 8 layers (zeros otherwise):
//   narrow  mb, stride, waves, lds_bytes
//   wide    rows, stride, lds_bytes
//   fleet   mb, nbuf, img2_off, waves, stride, lds_bytes
#include "sml_dense_fleet_fwd.h"
#include "sml_dense_fwd_plan.h"
#include "sml_dense_fwdw_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace {

std::vector<int> ints_of(const std::string& list) {
  std::vector<int> v;
  std::istringstream in(list);
  for (std::string w; std::getline(in, w, ',');) v.push_back(std::stoi(w));
  return v;
}

// 0, or 2 for a line that is no case
int answer(const std::string& mode, const std::string& line) {
  using namespace sml;
  std::istringstream in(line);
  std::string ws, as;
  long long score = 0, n = mode == "wide" ? (long long)DFWW_ROWS_SMALL : 1;
  if (!(in >> ws >> as)) return 2;
  in >> score >> n;
  const std::vector<int> widths = ints_of(ws), acts = ints_of(as);
  if (widths.empty() || acts.size() + 1 != widths.size()) return 2;
  const int nl = (int)acts.size(), D = widths[0];
  std::vector<DenseFwdLayer> L((size_t)(nl > 0 ? nl : 1));
  for (int l = 0; l < nl; ++l) L[(size_t)l] = DenseFwdLayer{widths[(size_t)l], widths[(size_t)l + 1], acts[(size_t)l], 0, 0};
  const bool planned = nl >= 1 && nl <= DFW_MAXLAYERS;
  if (mode == "wide") {
    const int img = dense_fwdw_image_offsets(L.data(), nl);
    const DenseFwdWPlan P = planned ? dense_fwdw_plan(L.data(), nl, (int)n) : DenseFwdWPlan{};
    std::printf("%s\t%d\t%d\t%d\t%d\n", dense_fwdw_check(L.data(), nl, D, img, score != 0).c_str(), img, P.rows, P.stride,
                P.lds_bytes);
    return 0;
  }
  const int img = dense_fwd_image_offsets(L.data(), nl);
  if (mode == "narrow") {
    const DenseFwdPlan P = planned ? dense_fwd_plan(L.data(), nl, D) : DenseFwdPlan{};
    std::printf("%s\t%d\t%d\t%d\t%d\t%d\n", dense_fwd_check(L.data(), nl, D, img, score != 0).c_str(), img, P.mb, P.stride,
                P.waves, P.lds_bytes);
    return 0;
  }
  const DenseFleetFwdPlan F = planned ? dense_fleet_fwd_plan(L.data(), nl, D) : DenseFleetFwdPlan{};
  std::printf("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n",
              dense_fleet_fwd_check(L.data(), nl, D, img, score != 0, n, nullptr, 0, -1).c_str(), img, F.one.mb, F.nbuf,
              F.img2_off, F.waves, F.one.stride, F.one.lds_bytes);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode != "narrow" && mode != "wide" && mode != "fleet") {
    std::fprintf(stderr, "usage: dense_fwd_check narrow|wide|fleet [widths acts [score [n]]]\n");
    return 2;
  }
  std::string line;
  if (argc > 2) {
    for (int i = 2; i < argc; ++i) line += std::string(argv[i]) + " ";
    return answer(mode, line);
  }
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    if (answer(mode, line)) {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
