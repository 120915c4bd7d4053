// Host check of the lane-masked transposed-read address table (include/sml_common.h):
// tr_wr_off, tr_rd_off, tr_rd_off_half and the cell words, as the XP 5 packed-pair loop of
// kernels/ae_fused.hip uses them.  Compiled as HIP, host side only; needs no GPU.
//
// ds_read_b64_tr_b16 is emulated per 16-lane group: every lane loads 8 bytes (four bf16) from its
// own address, and result lane c, element q, is element c & 3 of what source lane 4q + (c >> 2)
// loaded.  A wave's twelve 512-B slots are filled through tr_wr_off with distinct values, the cell
// area sits where the kernel puts it (past the slots, the masked slots being 9, 10, 11), and for
// every lane the reads through the two masked addresses must equal the select form they replace.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sml_common.h"

namespace {

constexpr int TS = 12, SLOT0 = 9;                 // slots per wave, first masked slot
constexpr int SCR = TS * 512;                     // one wave's transpose scratch
constexpr int WAVES = 4, GAP = 256 + 4 * 3648;    // the normaliser and the rings lie between
constexpr int CELLS_OFF = WAVES * SCR + GAP;      // workgroup offset of the cell area
constexpr int BYTES = CELLS_OFF + sml::TR_MASK_CELL_BYTES;

struct Quad {
  uint16_t v[4];
};

Quad load8(const std::vector<uint8_t>& lds, int addr, int* oob) {
  Quad q{};
  if (addr < 0 || addr + 8 > (int)lds.size() || (addr & 7)) {
    ++*oob;
    return q;
  }
  std::memcpy(q.v, lds.data() + addr, 8);
  return q;
}

// the transposed read of one wave: addr[lane] -> result[lane]
void tr_read_wave(const std::vector<uint8_t>& lds, const int (&addr)[64], Quad (&out)[64], int* oob) {
  Quad src[64];
  for (int l = 0; l < 64; ++l) src[l] = load8(lds, addr[l], oob);
  for (int l = 0; l < 64; ++l) {
    const int c = l & 15, base = l & ~15;
    for (int q = 0; q < 4; ++q) out[l].v[q] = src[base + 4 * q + (c >> 2)].v[c & 3];
  }
}

uint16_t tile_value(int wave, int slot, int f, int r) {
  if (slot == SLOT0 && f == 1) return 0x3F80;   // the bias input: bf16 1.0 in every row
  return (uint16_t)(1 + (wave * TS + slot) * 256 + f * 16 + r);   // distinct over the workgroup, never 0
}

}  // namespace

int main() {
  std::vector<uint8_t> lds(BYTES, 0xAB);   // poison: a read of anything unwritten shows
  // the cells, as the kernel's prologue writes them
  for (int i = 0; i < sml::TR_MASK_CELL_BYTES / 4; ++i) {
    const unsigned w = sml::tr_mask_cell_word(i);
    std::memcpy(lds.data() + CELLS_OFF + 4 * i, &w, 4);
  }
  // every wave's slots, feature-major: lane (c, g) holds P[f = 4g + i][r = c]
  for (int w = 0; w < WAVES; ++w)
    for (int s = 0; s < TS; ++s)
      for (int l = 0; l < 64; ++l) {
        const int c = l & 15, g = l >> 4;
        Quad q;
        for (int i = 0; i < 4; ++i) q.v[i] = tile_value(w, s, 4 * g + i, c);
        std::memcpy(lds.data() + w * SCR + s * 512 + sml::tr_wr_off(c, g), q.v, 8);
      }
  int bad = 0, oob = 0;
  for (int w = 0; w < WAVES; ++w) {
    const int scr = w * SCR;
    const int cells = CELLS_OFF - SLOT0 * 512 - w * SCR;   // from this wave's slot (the kernel's expression)
    for (int s = 0; s < TS; ++s) {
      int a_full[64], a_half[2][64];
      for (int l = 0; l < 64; ++l) {
        const int c = l & 15, g = l >> 4;
        a_full[l] = scr + sml::tr_rd_off(c, g) + s * 512;
        for (int h = 0; h < 2; ++h) a_half[h][l] = scr + sml::tr_rd_off_half(c, g, h, cells) + s * 512;
      }
      Quad full[64], half[2][64];
      tr_read_wave(lds, a_full, full, &oob);
      for (int l = 0; l < 64; ++l) {   // the plain read: P[f = c][r = 4g + q]
        const int c = l & 15, g = l >> 4;
        for (int q = 0; q < 4; ++q) bad += full[l].v[q] != tile_value(w, s, c, 4 * g + q);
      }
      if (s < SLOT0 || s > SLOT0 + 2) continue;   // only the masked slots have cells
      for (int h = 0; h < 2; ++h) tr_read_wave(lds, a_half[h], half[h], &oob);
      for (int l = 0; l < 64; ++l) {
        const int c = l & 15;
        const bool lo = c < 8;
        // the select form: (lo ? x : 0) and (lo ? 0 : x); the xub slot's second half keeps c == 1
        const bool keep0 = lo, keep1 = !lo || (s == SLOT0 && c == 1);
        for (int q = 0; q < 4; ++q) {
          const uint16_t want0 = keep0 ? full[l].v[q] : 0, want1 = keep1 ? full[l].v[q] : 0;
          if (half[0][l].v[q] != want0 || half[1][l].v[q] != want1) {
            if (bad < 8)
              std::printf("wave %d slot %d lane %d q %d: got %04x %04x want %04x %04x\n", w, s, l, q, half[0][l].v[q],
                          half[1][l].v[q], want0, want1);
            ++bad;
          }
        }
      }
    }
  }
  std::printf("%s tr_mask_table: %d mismatches, %d out-of-range or misaligned reads\n", (bad || oob) ? "FAIL" : "PASS", bad,
              oob);
  return (bad || oob) ? 1 : 0;
}
