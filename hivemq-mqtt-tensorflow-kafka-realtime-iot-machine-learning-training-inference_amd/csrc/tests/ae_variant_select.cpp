// Host walk of the AE train launcher's choice (include/sml_ae_variants.h): for a fixed grid of
// launch requests and SML_AE_* knob settings, one line per case with the request, the knobs, and
// either REFUSE or the chosen variant's name, its eleven values, the grid it gets on 256 CUs for a
// caller's grid of 2560, and the (XP, TS) ae_train_last_variant would report.  Plain C++, no GPU.
// tests/test_ae_variant_select.py holds the output to tests/golden/ae_variant_select.txt, which
// was recorded from the if / else chain this table replaced.
//
// The grid is thinned, not a full cross product, to keep the golden file readable.  Requests come
// in classes (no ring possible; a ring at D != 18; D = 18 without a packed ring; D = 18 with one,
// with an even or odd tile count; requests refused whatever the knobs say), and each class meets
// the groups of knob settings that can influence it (MIN, TILE, DIRECT, PAIR below), every value
// of every knob among them.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sml_ae_variants.h"

using namespace sml;

namespace {

constexpr int CUS = 256, GRID_IN = 2560;   // between the one-tile cap (2048) and the 4-wave pair cap (3072)
constexpr unsigned OTHER_LIVE = 0x3FFF0u;  // neither full nor the cardata set

AETrainKnobs defaults() {
  AETrainKnobs k{};
  k.ring = true; k.rounds = 3; k.direct_occ = 4; k.ilp = 3; k.direct_pairs = true;
  k.pair_occ = 4; k.pair_xp = 5; k.occ = 4;
  return k;
}

AETrainRequest base_request(int D) {
  AETrainRequest r{};
  r.pack = PACK_REF; r.D = D; r.n1 = 14; r.n2 = 7; r.n3 = 7;
  r.n = 64; r.ld = D; r.want_acc = true; r.has_cursor = false; r.has_xpack = false;
  r.x_addr = 0; r.xpack_addr = 0; r.xpack_live = 0;
  return r;
}

void emit(const AETrainRequest& r, const AETrainKnobs& k) {
  const char* live = r.xpack_live == 0 ? "0" : r.xpack_live == kLiveCardata ? "cardata"
                   : r.xpack_live == OTHER_LIVE ? "other" : "full";
  std::printf("D=%d n=%lld ld=%lld xa=%u cur=%d xpack=%s acc=%d live=%s w=%d/%d/%d pack=%d | "
              "ilp=%d pocc=%d pxp=%d occ=%d dp=%d docc=%d ring=%d rounds=%d -> ",   // SML_AE_ILP, _PAIR_OCC, _PAIR_XP, ...
              r.D, (long long)r.n, (long long)r.ld, r.x_addr, (int)r.has_cursor,
              !r.has_xpack ? "null" : r.xpack_addr ? "odd" : "ok", (int)r.want_acc, live, r.n1, r.n2, r.n3, r.pack,
              k.ilp, k.pair_occ, k.pair_xp, k.occ, (int)k.direct_pairs, k.direct_occ, (int)k.ring, k.rounds);
  const AEVariantRow* v = ae_train_select(r, k);
  if (v == nullptr) {
    std::printf("REFUSE\n");
    return;
  }
  const int cap = ae_train_grid_cap(*v, k, CUS);
  std::printf("%s <%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d> grid=%d note=(%d,%d)\n", v->name, v->PACK, v->VEC, v->PF, v->OCC,
              v->DC, v->XM, v->ILP, v->TS, v->NPW, v->XP, v->CM, GRID_IN < cap ? GRID_IN : cap, v->xp_noted, v->ts_noted);
}

// the knob settings every request meets, in groups: a request meets the groups that can influence
// its class.  Each knob's values alone, and the pairs of knobs that one condition reads together.
enum : unsigned {
  MIN = 1,        // default, SML_AE_OCC=3, SML_AE_RING=0
  TILE = 2,       // SML_AE_ILP 1 / 2 with SML_AE_OCC 3 / 4, SML_AE_ROUNDS=1
  DIRECT = 4,     // SML_AE_DIRECT_PAIRS=0, SML_AE_DIRECT_OCC=3 with every SML_AE_PAIR_XP
  PAIR_OCC = 8,   // SML_AE_PAIR_OCC 2 / 3
  PAIR = 16,      // SML_AE_PAIR_OCC x SML_AE_PAIR_XP (XP 5, the default, is in MIN and PAIR_OCC)
};
struct KnobCase {
  unsigned group;
  AETrainKnobs k;
};
std::vector<KnobCase> knob_cases() {
  std::vector<KnobCase> out;
  auto add = [&](unsigned group, auto&& set) {
    AETrainKnobs k = defaults();
    set(k);
    out.push_back({group, k});
  };
  add(MIN, [](AETrainKnobs&) {});
  add(MIN, [](AETrainKnobs& k) { k.occ = 3; });
  add(MIN, [](AETrainKnobs& k) { k.ring = false; });
  for (int ilp = 1; ilp <= 2; ++ilp)
    for (int occ = 3; occ <= 4; ++occ) add(TILE, [&](AETrainKnobs& k) { k.ilp = ilp; k.occ = occ; });
  add(TILE, [](AETrainKnobs& k) { k.ilp = 2; k.rounds = 1; });
  add(TILE, [](AETrainKnobs& k) { k.rounds = 1; });
  add(TILE, [](AETrainKnobs& k) { k.occ = 3; k.rounds = 1; });
  add(DIRECT, [](AETrainKnobs& k) { k.direct_pairs = false; });
  for (int xp = 0; xp <= 5; ++xp) add(DIRECT, [&](AETrainKnobs& k) { k.direct_occ = 3; k.pair_xp = xp; });
  add(DIRECT, [](AETrainKnobs& k) { k.direct_occ = 3; k.rounds = 1; });
  for (int po = 2; po <= 3; ++po) add(PAIR_OCC, [&](AETrainKnobs& k) { k.pair_occ = po; });
  add(PAIR_OCC, [](AETrainKnobs& k) { k.pair_occ = 2; k.rounds = 1; });
  for (int po = 2; po <= 4; ++po)
    for (int xp = 0; xp <= 4; ++xp) add(PAIR, [&](AETrainKnobs& k) { k.pair_occ = po; k.pair_xp = xp; });
  return out;
}

int walk() {
  const std::vector<KnobCase> cases = knob_cases();
  int lines = 0;
  auto run = [&](const AETrainRequest& r, unsigned groups) {
    for (const KnobCase& c : cases)
      if (c.group & groups) emit(r, c.k), ++lines;
  };
  const int64_t ROW_LIMIT = int64_t(1) << 35;   // the 32-bit pair count's limit
  // shapes, no packed ring: only D = 18 has more than the one-tile loops to choose from
  for (int D : {16, 17, 18, 20, 30, 31, 32})   // 20: the deepest 4-wave ring without the compile-time D
    for (int pad = 0; pad <= 2; pad += 2)
      for (unsigned xa : {0u, 8u, 4u}) {
        if ((pad || xa) && D != 17 && D != 18 && D != 30) continue;   // padding and alignment: an odd D, 18, a ring D
        AETrainRequest r = base_request(D);
        r.ld = D + pad; r.x_addr = xa;
        run(r, D == 18 && pad == 0 && xa == 0 ? MIN | TILE | DIRECT : MIN);
      }
  // 64: four tiles; 48: three; 49, 70: a ragged tile after three / four (49 * 18 is no multiple of 4)
  for (int D : {18, 30})
    for (int64_t n : {int64_t(64), int64_t(48), int64_t(49), int64_t(70), ROW_LIMIT})
      for (int cur = 0; cur <= 1; ++cur) {
        if (n == 64 && cur == 0) continue;   // above
        AETrainRequest r = base_request(D);
        r.n = n; r.has_cursor = cur != 0;
        run(r, D != 18 || n == ROW_LIMIT || n == 70 ? MIN : n == 64 ? MIN | TILE | DIRECT : MIN | TILE);
      }
  // D = 18 without a packed ring, where the mask and want_acc must not matter
  for (int acc = 0; acc <= 1; ++acc)
    for (unsigned live : {0u, kLiveCardata}) {
      if (live == 0 && acc == 1) continue;   // above
      AETrainRequest r = base_request(18);
      r.want_acc = acc != 0; r.xpack_live = live;
      run(r, MIN | TILE | DIRECT);
      r.n = 48;
      run(r, MIN);
    }
  // D = 18 with a packed ring: its tile count, alignment, want_acc and live mask
  for (int64_t n : {int64_t(64), int64_t(48), int64_t(49), int64_t(70), ROW_LIMIT})
    for (unsigned live : {0u, (1u << 18) - 1u, kLiveCardata, OTHER_LIVE}) {
      AETrainRequest r = base_request(18);
      r.n = n; r.has_xpack = true; r.xpack_live = live;
      const bool readable = live != OTHER_LIVE && n != ROW_LIMIT;
      run(r, !readable || n == 70 ? MIN : n == 64 ? MIN | TILE | PAIR_OCC | PAIR : MIN | TILE | PAIR_OCC);
      if ((n != 64 && n != 49) || (live != 0 && live != kLiveCardata)) continue;
      r.want_acc = false;
      run(r, n == 64 ? MIN | TILE : MIN);
      r.want_acc = true; r.xpack_addr = 8;
      run(r, n == 64 ? MIN | TILE : MIN);
    }
  const int widths[][3] = {{15, 7, 7}, {16, 7, 7}, {14, 8, 7}, {14, 7, 8}};   // the edge, and one past it per layer
  for (const auto& w : widths) {
    AETrainRequest r = base_request(18);
    r.n1 = w[0]; r.n2 = w[1]; r.n3 = w[2];
    run(r, MIN | DIRECT);
    r.has_xpack = true;
    for (unsigned live : {0u, kLiveCardata}) {
      r.xpack_live = live;
      run(r, live == 0 ? MIN | TILE | PAIR_OCC : MIN | PAIR_OCC);
    }
  }
  // a packed ring with a cursor, and at the other widths (full mask: D <= 31 only)
  for (int64_t n : {int64_t(64), int64_t(49)})
    for (unsigned live : {0u, kLiveCardata}) {
      AETrainRequest r = base_request(18);
      r.n = n; r.has_cursor = true; r.has_xpack = true; r.xpack_live = live;
      run(r, MIN | PAIR_OCC);
    }
  for (int D : {17, 30, 31, 32})
    for (unsigned live : {0u, D < 32 ? (1u << D) - 1u : 0xFFFFFFFFu, kLiveCardata, OTHER_LIVE}) {
      AETrainRequest r = base_request(D);
      r.has_xpack = true; r.xpack_live = live;
      run(r, MIN);
    }
  // other activations: the dynamic kernel whatever else is asked, the row limit included
  for (int D : {18, 17})
    for (int xs = 0; xs <= 1; ++xs)
      for (int64_t n : {int64_t(64), ROW_LIMIT}) {
        AETrainRequest r = base_request(D);
        r.pack = PACK_REF ^ 1; r.has_xpack = xs != 0; r.n = n; r.xpack_live = xs ? OTHER_LIVE : 0;
        run(r, MIN);
      }
  return lines;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && argv[1][0] == '-' && argv[1][1] == 't') {   // -t: the table itself
    for (const AEVariantRow& v : kAEVariants)
      std::printf("%s <%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d> %s note=(%d,%d)\n", v.name, v.PACK, v.VEC, v.PF, v.OCC, v.DC,
                  v.XM, v.ILP, v.TS, v.NPW, v.XP, v.CM, v.grid == AEGrid::Pairs ? "pairs" : "one-tile", v.xp_noted,
                  v.ts_noted);
    return 0;
  }
  return walk() > 0 ? 0 : 1;
}
