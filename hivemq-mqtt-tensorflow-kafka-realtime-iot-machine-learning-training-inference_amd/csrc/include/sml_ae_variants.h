// The instances of ae_train_kernel (kernels/ae_fused.hip) as named types, the table of them, and
// the choice among them as a pure function of the launch request and the SML_AE_* knobs.
// Plain C++17 with no HIP and no getenv, so a host program can include it and walk the choice
// without a GPU (csrc/tests/ae_variant_select.cpp).  What PF, OCC, TS, NPW, XP and CM mean is written
// where the kernel uses them; here is only which combinations are built and when each one runs.
#pragma once

#include <cstdint>

namespace sml {

// Activation codes packed as a1 | a2 << 2 | a3 << 4 | a4 << 6 (Act of sml_common.h); the
// reference model is tanh, relu, tanh, relu.  PACK_DYN: the codes are read at run time.
constexpr int PACK_REF = 2 | (1 << 2) | (2 << 4) | (1 << 6);
constexpr int PACK_DYN = -1;
// xpack_live of the cardata normaliser: it zeroes features 0, 2, 4 and 5 of the 18
constexpr unsigned kLiveCardata = 0x3FFFFu & ~((1u << 0) | (1u << 2) | (1u << 4) | (1u << 5));
// per-wave ring bytes of the one-tile ring variants (ring_bytes<4>() / ring_bytes<3>() of the kernel file)
constexpr int kRing1Tile4w = 3968, kRing1Tile3w = 6144;

// How the launcher caps the grid: two rounds of the SML_AE_OCC residency (the one-tile loops), or
// SML_AE_ROUNDS rounds of the variant's own OCC workgroups per CU (the tile-pair loops).
enum class AEGrid { OneTile, Pairs };

// ---- the variants: ae_train_kernel<V> reads V's eleven values ---------------------------------
namespace aev {
struct AEVariantBase {
  static constexpr int DC = 0, XM = 0, ILP = 1, TS = 10, NPW = 1, XP = 0, CM = 0;
  static constexpr AEGrid GRID = AEGrid::OneTile;
  static constexpr bool NOTED = false;   // ae_train_last_variant reports this variant's (XP, TS)
};
struct AERefVec : AEVariantBase {   // the reference activations, 8-byte row reads
  static constexpr int PACK = PACK_REF;
  static constexpr bool VEC = true;
};

// one tile per trip, any activations / any D: one tile of register prefetch
struct Dynamic : AEVariantBase {
  static constexpr int PACK = PACK_DYN, PF = 0, OCC = 3;
  static constexpr bool VEC = false;
};
struct RegPrefetch : AERefVec {
  static constexpr int PF = 0, OCC = 3;
  static constexpr bool VEC = false;
};
struct RegPrefetchVec : AERefVec { static constexpr int PF = 0, OCC = 3; };
// one tile per trip from the LDS-DMA ring, the deepest ring that fits D
struct OneTileRing3w_PF3 : AERefVec { static constexpr int PF = 3, OCC = 3; };
struct OneTileRing3w_PF5 : AERefVec { static constexpr int PF = 5, OCC = 3; };
struct OneTileRing4w_PF2 : AERefVec { static constexpr int PF = 2, OCC = 4; };
struct OneTileRing4w_PF3 : AERefVec { static constexpr int PF = 3, OCC = 4; };
// the cardata-v1 reference model: D fixed at compile time
struct OneTileRing4w_D18 : OneTileRing4w_PF3 { static constexpr int DC = 18; };
// ... on the tile-packed ring (rows normalised and argmax(x) taken at ingest)
struct OneTilePacked4w_D18 : OneTileRing4w_D18 { static constexpr int XM = 1; };
// SML_AE_ILP=2: tile pairs (t, t + stride) of the tile-packed ring
struct TilePair3w : AERefVec {
  static constexpr int PF = 6, OCC = 3, DC = 18, XM = 1, ILP = 2;
  static constexpr AEGrid GRID = AEGrid::Pairs;
};

// packed pairs (SML_AE_ILP=3) on the 18-column tile-packed ring.  The 3-wave builds take every
// XP 0..3; the 4-wave build needs the early writes' registers (XP 0 means 1) and XP 2 spills
// there (the MFMA-transpose temporaries), so it has XP 1 and XP 3.
struct Pair18col : AERefVec {
  static constexpr int DC = 18, XM = 1, ILP = 3;
  static constexpr AEGrid GRID = AEGrid::Pairs;
};
struct Pair18col3w : Pair18col { static constexpr int PF = 6, OCC = 3; };
struct Pair18col4w : Pair18col { static constexpr int PF = 4, OCC = 4; };
struct Pair18col3w_XP0 : Pair18col3w {};
struct Pair18col3w_XP1 : Pair18col3w { static constexpr int XP = 1; };
struct Pair18col3w_XP2 : Pair18col3w { static constexpr int XP = 2; };
struct Pair18col3w_XP3 : Pair18col3w { static constexpr int XP = 3; };
struct Pair18col4w_XP1 : Pair18col4w { static constexpr int XP = 1; };
struct Pair18col4w_XP3 : Pair18col4w { static constexpr int XP = 3; };
// two packed pairs per iteration, 2 waves / SIMD
struct Pair18col2w_NPW2 : Pair18col { static constexpr int PF = 8, OCC = 2, NPW = 2; };

// the compact-ring twin of every packed-pair variant above, and the XP 4 and XP 5 instances,
// which are built for the compact ring at 4 waves only
struct PairCompact3w_XP0 : Pair18col3w_XP0 { static constexpr int CM = 1; };
struct PairCompact3w_XP1 : Pair18col3w_XP1 { static constexpr int CM = 1; };
struct PairCompact3w_XP2 : Pair18col3w_XP2 { static constexpr int CM = 1; };
struct PairCompact3w_XP3 : Pair18col3w_XP3 { static constexpr int CM = 1; };
struct PairCompact2w_NPW2 : Pair18col2w_NPW2 { static constexpr int CM = 1; };
struct PairCompact4w : Pair18col4w {
  static constexpr int CM = 1;
  static constexpr bool NOTED = true;
};
struct PairCompact4w_XP1 : PairCompact4w {
  static constexpr int XP = 1;
  static constexpr bool NOTED = false;
};
struct PairCompact4w_XP3 : PairCompact4w { static constexpr int XP = 3; };
// TS 12: 39 424 B, still four workgroups per CU
struct PairCompact4w_XP4 : PairCompact4w { static constexpr int TS = 12, XP = 4; };
// XP 4 with the lane masks in the read addresses: 40 480 B
struct PairCompact4w_XP5 : PairCompact4w { static constexpr int TS = 12, XP = 5; };

// rows trained once (fresh / streamed): packed pairs straight from the raw rows,
// normalize_fn + argmax(x) in registers (no K8 pack pass)
struct DirectPair : AERefVec {
  static constexpr int DC = 18, ILP = 3;
  static constexpr AEGrid GRID = AEGrid::Pairs;
};
struct DirectPair3w_XP0 : DirectPair { static constexpr int PF = 6, OCC = 3; };
struct DirectPair3w_XP3 : DirectPair3w_XP0 { static constexpr int XP = 3; };
struct DirectPair4w_XP3 : DirectPair { static constexpr int PF = 4, OCC = 4, XP = 3; };
}  // namespace aev

// ---- the table ----------------------------------------------------------------------------------
// One line per built instance; the kernel file takes its kernel pointers from the same list.
#define SML_AE_TRAIN_VARIANTS(X)                                                                        \
  X(Dynamic) X(RegPrefetch) X(RegPrefetchVec)                                                           \
  X(OneTileRing3w_PF3) X(OneTileRing3w_PF5) X(OneTileRing4w_PF2) X(OneTileRing4w_PF3)                   \
  X(OneTileRing4w_D18) X(OneTilePacked4w_D18) X(TilePair3w)                                             \
  X(Pair18col3w_XP0) X(Pair18col3w_XP1) X(Pair18col3w_XP2) X(Pair18col3w_XP3)                           \
  X(Pair18col4w_XP1) X(Pair18col4w_XP3) X(Pair18col2w_NPW2)                                             \
  X(PairCompact3w_XP0) X(PairCompact3w_XP1) X(PairCompact3w_XP2) X(PairCompact3w_XP3)                   \
  X(PairCompact4w_XP1) X(PairCompact4w_XP3) X(PairCompact4w_XP4) X(PairCompact4w_XP5)                   \
  X(PairCompact2w_NPW2)                                                                                 \
  X(DirectPair3w_XP0) X(DirectPair3w_XP3) X(DirectPair4w_XP3)

struct AEVariantRow {
  const char* name;
  int PACK, VEC, PF, OCC, DC, XM, ILP, TS, NPW, XP, CM;
  AEGrid grid;
  int xp_noted, ts_noted;   // what ae_train_last_variant reports (-1, -1 unless NOTED)
};
template <class V>
constexpr AEVariantRow ae_variant_row(const char* name) {
  return {name,  V::PACK, V::VEC, V::PF, V::OCC, V::DC,  V::XM, V::ILP,
          V::TS, V::NPW,  V::XP,  V::CM, V::GRID, V::NOTED ? V::XP : -1, V::NOTED ? V::TS : -1};
}
#define SML_AE_ROW(V) ae_variant_row<aev::V>(#V),
inline constexpr AEVariantRow kAEVariants[] = {SML_AE_TRAIN_VARIANTS(SML_AE_ROW)};
#undef SML_AE_ROW
#define SML_AE_ID(V) V,
enum class AEVariantId : int { SML_AE_TRAIN_VARIANTS(SML_AE_ID) };   // a row's index in kAEVariants
#undef SML_AE_ID
constexpr int kAEVariantCount = sizeof(kAEVariants) / sizeof(kAEVariants[0]);

// ---- the choice ---------------------------------------------------------------------------------
// Every SML_AE_* variable the launcher looks at, parsed (ae_train_knobs of the kernel file).
struct AETrainKnobs {
  bool ring;           // SML_AE_RING: the LDS-DMA ring (false: register prefetch)
  int rounds;          // SML_AE_ROUNDS: residency rounds of the tile-pair grids, 1..8
  int direct_occ;      // SML_AE_DIRECT_OCC: waves per SIMD of the direct packed-pair step, 3 | 4
  int ilp;             // SML_AE_ILP: 1 one tile, 2 tile pairs, 3 packed pairs
  bool direct_pairs;   // SML_AE_DIRECT_PAIRS: raw rows on the packed-pair loop
  int pair_occ;        // SML_AE_PAIR_OCC: waves per SIMD of the packed-pair loop, 2 | 3 | 4
  int pair_xp;         // SML_AE_PAIR_XP: the packed-pair weight-gradient operand path, 0..5
  int occ;             // SML_AE_OCC: waves per SIMD of the one-tile ring loop, 3 | 4
};

// What ae_train_launch was asked for, as far as the choice depends on it.
struct AETrainRequest {
  int pack;              // the four activation codes, packed like PACK_REF
  int D, n1, n2, n3;
  int64_t n, ld;
  bool want_acc, has_cursor, has_xpack;
  unsigned x_addr, xpack_addr;   // the low four address bits of x and of xpack
  unsigned xpack_live;           // the features the packed ring stores (0 = all D)
};

// The row of kAEVariants to launch, or nullptr where the launcher refuses (hipErrorInvalidValue).
inline const AEVariantRow* ae_train_select(const AETrainRequest& r, const AETrainKnobs& k) {
  auto packed_pair = [](int xm, int cm, int occ, int xp) -> const AEVariantRow* {
    for (const AEVariantRow& v : kAEVariants)
      if (v.ILP == 3 && v.XM == xm && v.CM == cm && v.OCC == occ && v.XP == xp) return &v;
    return nullptr;
  };
  using Id = AEVariantId;
  auto row = [](Id id) { return &kAEVariants[(int)id]; };
  if (r.pack != PACK_REF) return row(Id::Dynamic);
  const int D = r.D;
  const bool vec = (r.ld & 1) == 0 && (D & 1) == 0 && D >= 2 && (r.x_addr & 7) == 0;
  // LDS-DMA ring: contiguous rows, 17 <= D <= 31 (two DMAs per tile), 16-B aligned
  // tiles (the ring cursor moves in whole batches, so n * ld * 4 must stay 16-B aligned)
  const bool ring_ok = vec && r.ld == D && D >= 17 && D <= 31 && (r.x_addr & 15) == 0 &&
                       (!r.has_cursor || ((r.n * r.ld) & 3) == 0) && k.ring;
  const bool ring18 = ring_ok && D == 18;
  // tile-packed ring with ingest-time x argmax (pack_tiles_argmax): whole 16-row tiles
  const bool xa_ok = r.has_xpack && r.want_acc && (r.n & 15) == 0 && (r.xpack_addr & 15) == 0;
  // the pair loops count pairs in 32 bits (2^30 pairs = 2^35 rows: past any device's memory)
  if ((r.n >> 5) >= (int64_t(1) << 30)) return nullptr;
  // packed pairs: an even number of whole tiles, the narrow layers packed two tiles to a fragment
  const bool pairs_ok = (r.n & 31) == 0 && k.ilp == 3 && r.n1 <= 15 && r.n2 <= 7 && r.n3 <= 7;
  // xpack_live: the features the packed ring stores (0 = all D).  Only the packed-pair variants
  // read the compact ring of the cardata live set; any other mask, or any other variant, is refused.
  // That mask means the LANE-ORDERED compact layout (pack_tiles_argmax with lane_order, what
  // FusedAE builds): no kernel reads the ascending compact layout.
  const bool full = r.xpack_live == 0 || (D <= 31 && r.xpack_live == (1u << D) - 1u);
  const bool cm = !full && D == 18 && r.xpack_live == kLiveCardata;
  if (r.has_xpack && !full && !cm) return nullptr;
  // A caller that passes a tile-packed ring may have packed it from rows other than x's (an
  // epoch's shuffle fused into the pack: FusedAE.pack_ring); only the XM 1 variants read it,
  // so refuse to silently train on x when none of them applies.
  const bool packed = ring18 && xa_ok;
  const AEVariantRow* v = nullptr;
  if (packed && k.ilp == 2 && !cm) {
    v = row(Id::TilePair3w);
  } else if (packed && pairs_ok) {
    // the operand path each build has: 4 and 5 on the compact ring at 4 waves only (3 elsewhere)
    const int po = k.pair_occ, xp = k.pair_xp;
    const int eff = po == 2 ? 0 : po == 3 ? (xp >= 3 ? 3 : xp) : (cm && xp >= 4) ? xp : xp >= 2 ? 3 : 1;
    v = packed_pair(1, cm, po, eff);
  } else if (packed && k.occ == 4 && !cm) {
    v = row(Id::OneTilePacked4w_D18);
  }
  if (r.has_xpack) return v;   // nullptr: no reading variant applies
  if (ring18 && pairs_ok && k.direct_pairs)
    // SML_AE_PAIR_XP picks only the 3-wave build's path; the 4-wave one (the default) is XP 3
    return packed_pair(0, 0, k.direct_occ, (k.direct_occ == 4 || k.pair_xp >= 3) ? 3 : 0);
  if (ring18 && k.occ == 4) return row(Id::OneTileRing4w_D18);
  if (ring_ok && k.occ == 4) return row(3 * 64 * D <= kRing1Tile4w ? Id::OneTileRing4w_PF3 : Id::OneTileRing4w_PF2);
  if (ring_ok) return row(5 * 64 * D <= kRing1Tile3w ? Id::OneTileRing3w_PF5 : Id::OneTileRing3w_PF3);
  return row(vec ? Id::RegPrefetchVec : Id::RegPrefetch);
}

// The grid ae_train_launch uses: the caller's, capped at the variant's rounds x residency.
inline int ae_train_grid_cap(const AEVariantRow& v, const AETrainKnobs& k, int cus) {
  return (v.grid == AEGrid::Pairs ? k.rounds * v.OCC : 2 * k.occ) * cus;
}

}  // namespace sml
