// Stand-alone host program behind tests/test_tri_split.py: the split of the triangular inverse's problem list
// (bobe_amd/csrc/tri_split.hpp) for nb = 1 .. 70.  Built with the host compiler under -fsanitize=address,undefined.
// Exit status 0 and "ok <nb range>" on success; the first violated property otherwise.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../bobe_amd/csrc/tri_split.hpp"

using namespace bobe;

static int fails = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      std::printf("nb=%d: %s: ", nb, #cond);      \
      std::printf(__VA_ARGS__);                   \
      std::printf("\n");                          \
      if (++fails > 20) std::exit(1);             \
    }                                             \
  } while (0)

static int blocks(const TriProb& p) { return (p.hi - p.mid) * (p.mid - p.lo); }

int main() {
  for (int nb = 1; nb <= 70; ++nb) {
    const TriSplit s = tri_split(nb);
    const int nd = (int)s.depths.size();
    CHECK((int)s.lead.size() == nd && (int)s.trail.size() == nd, "%zu %zu %d", s.lead.size(), s.trail.size(), nd);
    if (nb == 1) {                               // nothing to invert beyond the block itself: no fork
      CHECK(s.mid == 0 && nd == 0 && s.table.empty(), "mid %d depths %d", s.mid, nd);
      continue;
    }
    CHECK(s.mid == nb / 2 && s.mid >= 1 && s.mid < nb, "mid %d", s.mid);
    // the top: exactly the problem {0, mid, nb}, in neither half
    CHECK(s.depths[0].count == 1 && s.lead[0].count == 0 && s.trail[0].count == 0, "top level");
    const TriProb top = s.table[s.depths[0].first];
    CHECK(top.lo == 0 && top.mid == s.mid && top.hi == nb && top.off == 0, "{%d %d %d %d}", top.lo, top.mid, top.hi, top.off);
    // the diagonal blocks: [0, mid) and [mid, nb) partition [0, nb) (trtri_part's k_trti_diag launches)
    std::vector<int> inverted(nb, 0);            // block -> 1 leading, 2 trailing
    for (int b = 0; b < s.mid; ++b) inverted[b] += 1;
    for (int b = s.mid; b < nb; ++b) inverted[b] += 2;
    int whole_total = 0, part_total = 0;
    for (int dd = 0; dd < nd; ++dd) {
      const Depth D = s.depths[dd], Ld = s.lead[dd], Td = s.trail[dd];
      CHECK(D.first >= 0 && D.first + D.count <= (int)s.table.size(), "depth %d", dd);
      CHECK(Td.first >= 0 && Td.first + Td.count <= (int)s.table.size(), "depth %d", dd);
      // the whole level: ascending lo, tile ranges back to back from 0
      int off = 0;
      for (int q = 0; q < D.count; ++q) {
        const TriProb p = s.table[D.first + q];
        CHECK(p.lo < p.mid && p.mid < p.hi && p.lo >= 0 && p.hi <= nb, "depth %d problem %d", dd, q);
        CHECK(q == 0 || p.lo >= s.table[D.first + q - 1].hi, "depth %d problem %d: not ascending", dd, q);
        CHECK(p.off == off, "depth %d problem %d: off %d, expected %d", dd, q, p.off, off);
        off += blocks(p);
      }
      CHECK(off == D.nblocks, "depth %d: %d blocks, %d listed", dd, off, D.nblocks);
      whole_total += D.nblocks;
      if (dd == 0) continue;
      // leading + trailing partition the level's list: the prefix and the rest
      CHECK(Ld.first == D.first && Ld.count + Td.count == D.count, "depth %d: %d + %d of %d", dd, Ld.count, Td.count, D.count);
      CHECK(Ld.nblocks + Td.nblocks == D.nblocks, "depth %d: %d + %d blocks of %d", dd, Ld.nblocks, Td.nblocks, D.nblocks);
      part_total += Ld.nblocks + Td.nblocks;
      off = 0;
      for (int q = 0; q < Ld.count; ++q) {       // the prefix lies in the leading half, numbered from 0 as it stands
        const TriProb p = s.table[Ld.first + q];
        CHECK(p.hi <= s.mid, "depth %d: leading problem %d reaches block %d", dd, q, p.hi);
        CHECK(p.off == off, "depth %d: leading problem %d off %d", dd, q, p.off);
        off += blocks(p);
      }
      CHECK(off == Ld.nblocks, "depth %d: leading tiles %d of %d", dd, off, Ld.nblocks);
      off = 0;
      for (int q = 0; q < Td.count; ++q) {       // the rest lies in the trailing half: the same problems, numbered from 0 again
        const TriProb p = s.table[Td.first + q], w = s.table[D.first + Ld.count + q];
        CHECK(p.lo >= s.mid, "depth %d: trailing problem %d starts at block %d", dd, q, p.lo);
        CHECK(p.lo == w.lo && p.mid == w.mid && p.hi == w.hi, "depth %d: trailing problem %d is another problem", dd, q);
        CHECK(p.off == off && w.off == off + Ld.nblocks, "depth %d: trailing problem %d off %d (whole level %d)", dd, q, p.off,
              w.off);
        off += blocks(p);
      }
      CHECK(off == Td.nblocks, "depth %d: trailing tiles %d of %d", dd, off, Td.nblocks);
      // the two parts' whole-level tile ranges [0, Ld.nblocks) and [Ld.nblocks, D.nblocks) are disjoint and cover the level
    }
    CHECK(whole_total - s.depths[0].nblocks == part_total, "%d vs %d", whole_total, part_total);
    // every strictly-lower 128-block of the inverse is written by exactly one problem, every diagonal one by one half
    std::vector<int> cover((size_t)nb * nb, 0);
    auto paint = [&](const TriProb& p) {
      for (int i = p.mid; i < p.hi; ++i)
        for (int j = p.lo; j < p.mid; ++j) cover[(size_t)i * nb + j]++;
    };
    paint(top);
    for (int dd = 1; dd < nd; ++dd) {
      for (int q = 0; q < s.lead[dd].count; ++q) paint(s.table[s.lead[dd].first + q]);
      for (int q = 0; q < s.trail[dd].count; ++q) paint(s.table[s.trail[dd].first + q]);
    }
    for (int i = 0; i < nb; ++i) {
      CHECK(inverted[i] == 1 || inverted[i] == 2, "diagonal block %d: %d", i, inverted[i]);
      for (int j = 0; j < i; ++j) CHECK(cover[(size_t)i * nb + j] == 1, "block (%d, %d) written %d times", i, j, cover[(size_t)i * nb + j]);
    }
  }
  if (fails) return 1;
  std::printf("ok 1..70\n");
  return 0;
}
