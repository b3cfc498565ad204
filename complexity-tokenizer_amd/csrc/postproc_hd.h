// The rules of the PostProcessor (the reference's src/postprocessors.rs:34-280), shared by the kernels
// (postproc.hip) and the CPU check (tools/postproc_check.cpp): plain integer code, no HIP include.
//
// A program is compiled (postproc_compile.cpp) into two flat lists of items, one for rows without a
// pair and one for rows with a pair.  An item copies the row's first sequence (A), its pair (B) or
// inserts one id (SPECIAL); the kind is not stored with the id, so nothing is in-band with an id.  A
// list carries prefix tables: pa[k], pb[k], ps[k] are the A, B and SPECIAL items before item k, and
// entry n holds the totals.  With na and nb the row's two lengths after truncation, item k starts at
// cell pa[k]*na + pb[k]*nb + ps[k] of the row, which does not decrease with k, so a cell finds its item
// by a binary search and the row's length is the same expression at n.
//
// No function reads outside the tables or the row it is given; every loop is a binary search.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PP_HD __host__ __device__ inline
#else
#define PP_HD inline
#endif

namespace postproc {

enum ItemKind : uint32_t { IT_A = 0, IT_B = 1, IT_SPECIAL = 2 };
enum Strategy : uint32_t { ONLY_FIRST = 0, ONLY_SECOND = 1, LONGEST_FIRST = 2 };  // ctok_postprocessor.h

constexpr uint32_t kMaxItems = 4096;  // CTOK_PP_MAX_ITEMS: a prefix count fits 16 bits
constexpr uint64_t kNoCell = ~0ull;

struct List {  // a compiled list (host or device pointers, or a workgroup's staged copy)
  const uint16_t* pa;   // n + 1 each
  const uint16_t* pb;
  const uint16_t* ps;
  const uint32_t* val;  // n: the id of a SPECIAL item
  uint32_t n;
};

struct In {  // a packed batch
  const uint32_t* ids;
  const uint64_t* off;  // n_rows + 1
  const uint32_t* pair_ids;
  const uint64_t* pair_off;  // n_rows + 1, or null: no row has a pair
  const uint8_t* has_pair;   // n_rows, or null: every row has a pair when pair_off is given
  uint64_t n_rows, n_ids, n_pair_ids;
};

struct Opts {
  uint32_t truncate, strategy;
  uint64_t truncate_to;
  uint32_t pad_left, pad_id;
};

struct Row {  // a row's two lengths after truncation
  uint32_t na, nb;
};

PP_HD bool row_has_pair(const In& in, uint64_t r) { return in.pair_off && (!in.has_pair || in.has_pair[r] != 0); }

// truncate (postprocessors.rs:209-254) in closed form.  longest_first pops one id at a time, from the
// first sequence while it is not the shorter: the longer one shrinks to the other's length, then
// the two take turns, the first sequence first.  tests/postproc_ref.py keeps the loop.
PP_HD void truncate(uint64_t na, uint64_t nb, bool has_pair, uint64_t max_len, uint32_t strategy, uint64_t* na_out,
                    uint64_t* nb_out) {
  *na_out = na;
  *nb_out = nb;
  const uint64_t total = na + nb;
  if (total <= max_len) return;
  const uint64_t rem = total - max_len;
  if (strategy == ONLY_FIRST) {
    *na_out = na - (rem < na ? rem : na);
  } else if (strategy == ONLY_SECOND) {
    if (has_pair) *nb_out = nb - (rem < nb ? rem : nb);
  } else {
    const uint64_t diff = na >= nb ? na - nb : nb - na;
    if (rem <= diff) {
      if (na >= nb) *na_out = na - rem;
      else *nb_out = nb - rem;
    } else {
      const uint64_t m = na < nb ? na : nb, rest = rem - diff;
      *na_out = m - (rest + 1) / 2;
      *nb_out = m - rest / 2;
    }
  }
}

PP_HD uint64_t item_pos(const List& l, uint32_t k, uint64_t na, uint64_t nb) {
  return (uint64_t)l.pa[k] * na + (uint64_t)l.pb[k] * nb + l.ps[k];
}

PP_HD uint64_t row_len(const List& l, uint64_t na, uint64_t nb) { return item_pos(l, l.n, na, nb); }

// the item of cell j < row_len: the last k with item_pos(k) <= j (an item of no cells is never it)
PP_HD uint32_t find_item(const List& l, uint64_t na, uint64_t nb, uint64_t j) {
  uint32_t lo = 0, hi = l.n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (item_pos(l, mid, na, nb) <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}

struct Cell {
  uint32_t kind;   // ItemKind
  uint32_t value;  // IT_SPECIAL: the id
  uint64_t at;     // IT_A, IT_B: the index within the row's sequence
};

PP_HD Cell cell_of(const List& l, uint64_t na, uint64_t nb, uint64_t j) {
  const uint32_t k = find_item(l, na, nb, j);
  Cell c;
  c.at = j - item_pos(l, k, na, nb);
  c.value = 0;
  if (l.pa[k + 1] != l.pa[k]) c.kind = IT_A;
  else if (l.pb[k + 1] != l.pb[k]) c.kind = IT_B;
  else {
    c.kind = IT_SPECIAL;
    c.value = l.val[k];
  }
  return c;
}

// the id of a cell
PP_HD uint32_t cell_id(const In& in, uint64_t r, const Cell& c) {
  if (c.kind == IT_A) return in.ids[in.off[r] + c.at];
  if (c.kind == IT_B) return in.pair_ids[in.pair_off[r] + c.at];
  return c.value;
}

// A row's part of the count: its lengths after truncation and its processed length.  *bad when its
// offsets are not in order (the row then has no cells, so nothing is read through them).
PP_HD uint64_t count_row(const In& in, const Opts& o, const List& single, const List& pair, uint64_t r, Row* row, bool* bad) {
  row->na = row->nb = 0;
  const uint64_t a0 = in.off[r], a1 = in.off[r + 1];
  bool wrong = a0 > a1 || a1 > in.n_ids || (r == 0 && a0 != 0) || (r + 1 == in.n_rows && a1 != in.n_ids);
  const bool hp = row_has_pair(in, r);
  uint64_t na = a1 - a0, nb = 0;
  if (hp) {
    const uint64_t b0 = in.pair_off[r], b1 = in.pair_off[r + 1];
    wrong = wrong || b0 > b1 || b1 > in.n_pair_ids;
    nb = b1 - b0;
  }
  if (wrong) {
    *bad = true;
    return 0;
  }
  if (o.truncate) truncate(na, nb, hp, o.truncate_to, o.strategy, &na, &nb);
  row->na = (uint32_t)na;  // (n_ids and n_pair_ids are below 2^32)
  row->nb = (uint32_t)nb;
  return row_len(hp ? pair : single, na, nb);
}

// the row of cell c of the ragged output: the last r in [lo, hi] with off[r] <= c (an empty row is never it)
PP_HD uint64_t find_row(const uint64_t* off, uint64_t lo, uint64_t hi, uint64_t c) {
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// pad (postprocessors.rs:266-280): the cell of the row that column col of the matrix shows, or kNoCell
PP_HD uint64_t matrix_cell(uint64_t width, uint64_t len, bool pad_left, uint64_t col) {
  if (!pad_left) return col < len ? col : kNoCell;
  const uint64_t pad = width - len;
  return col >= pad ? col - pad : kNoCell;
}

}  // namespace postproc
