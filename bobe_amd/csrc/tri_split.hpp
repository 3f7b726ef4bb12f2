// The problem list of the recursive triangular inverse (bobe_gp::trtri) and its split at the top level into a leading,
// a trailing and a top part.  Plain C++ without HIP: a pure function of the block count, which a stand-alone host program
// can include (tests/test_tri_split.py compiles one under the sanitizers).
#pragma once
#include <vector>

namespace bobe {

// problem {lo, mid, hi} of the recursive triangular inverse in 128-block units: with inv[lo:mid) and inv[mid:hi) known,
//   Tm = L[mid:hi, lo:mid) * inv[lo:mid)  (k_trtri_T),   inv[mid:hi, lo:mid) = -inv[mid:hi) * Tm  (k_trtri_R).
// `off` counts T x T tiles: a problem owns (hi-mid)(mid-lo)(128/T)^2 consecutive blocks.
struct TriProb { int lo, mid, hi, off; };

// problems [first, first + count) of the table: one launch pair; nblocks = the 128-blocks they own together
struct Depth { int first, count, nblocks; };

// table = every depth's problems in ascending lo (depths[dd]; depth 0 is the top problem {0, mid, nb}), followed by the
// TRAILING problems of the depths >= 1 once more with `off` restarting at 0 (trail[dd]).
// With mid = nb / 2 every problem below the top lies in one half: hi <= mid (leading: a prefix of its depth's list, whose
// `off` already start at 0 - lead[dd] points into the whole-level entries) or lo >= mid (trailing).  The leading part of the
// inverse is the diagonal blocks [0, mid), lead[dd] from the deepest depth up and the top problem's T; the trailing part the
// diagonal blocks [mid, nb) and trail[dd]; the top's R needs both.  lead[0] and trail[0] are empty; a depth may have no
// problem in one half (nb = 3: the leading half is a single block).  nb < 2: mid = 0, nothing to split.
struct TriSplit {
  std::vector<TriProb> table;
  std::vector<Depth> depths, lead, trail;
  int mid = 0;
};

inline TriSplit tri_split(int nb) {
  struct Item { int depth, lo, mid, hi; };
  std::vector<Item> items;
  struct Rec {
    static void go(std::vector<Item>& it, int depth, int lo, int hi) {
      if (hi - lo <= 1) return;
      const int mid = lo + (hi - lo) / 2;
      it.push_back({depth, lo, mid, hi});
      go(it, depth + 1, lo, mid);
      go(it, depth + 1, mid, hi);
    }
  };
  Rec::go(items, 0, 0, nb);
  TriSplit s;
  s.mid = nb >= 2 ? nb / 2 : 0;
  int maxd = -1;
  for (auto& i : items) maxd = i.depth > maxd ? i.depth : maxd;
  for (int dd = 0; dd <= maxd; ++dd) {
    Depth D{(int)s.table.size(), 0, 0}, Ld{D.first, 0, 0};
    for (auto& i : items)
      if (i.depth == dd) {
        const int blocks = (i.hi - i.mid) * (i.mid - i.lo);
        s.table.push_back({i.lo, i.mid, i.hi, D.nblocks});
        D.nblocks += blocks;
        D.count++;
        if (dd > 0 && i.hi <= s.mid) {
          Ld.nblocks += blocks;
          Ld.count++;
        }
      }
    s.depths.push_back(D);
    s.lead.push_back(Ld);
  }
  for (int dd = 0; dd <= maxd; ++dd) {
    const Depth D = s.depths[dd], Ld = s.lead[dd];
    Depth Td{(int)s.table.size(), 0, 0};
    for (int q = D.first + Ld.count; dd > 0 && q < D.first + D.count; ++q) {
      TriProb p = s.table[q];
      p.off -= Ld.nblocks;
      s.table.push_back(p);
      Td.nblocks += (p.hi - p.mid) * (p.mid - p.lo);
      Td.count++;
    }
    s.trail.push_back(Td);
  }
  return s;
}

}  // namespace bobe
