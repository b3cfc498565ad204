// CPU check of csrc/postproc_compile.cpp and csrc/postproc_hd.h, the PostProcessor's compiler and the
// rules behind csrc/postproc.hip: compiles a program and runs it over a packed batch the way the
// kernels' threads do -- a thread per row for the count, the scan, then a thread per cell in
// workgroups of 256 that stage the prefix tables first -- with every buffer exactly as long as what
// was counted, so that the address sanitizer sees an id too many.  Built by tests/test_postproc_cpu.py
// with g++ -fsanitize=address,undefined.
//
// stdin:  u64 n_steps, per step {u32 kind, flags, id_a, id_b; u64 single_len, pair_len, n_tok; single;
//         pair; per token {u64 len; u32 id; bytes}},
//         u32 truncate, strategy; u64 truncate_to; u32 padded, pad_left; u64 pad_to; u32 pad_id,
//         u32 pairs (0: none, 1: with has_pair, 2: every row), u64 n_rows, off[n_rows + 1],
//         when pairs: pair_off[n_rows + 1], when pairs == 1: has_pair[n_rows], the ids, the pair ids
// stdout: u64 items_single, items_pair, n, width; ragged: off[n_rows + 1], ids[n];
//         padded: row_len[n_rows] (u32), then ids, attention_mask, token_type_ids, special_tokens_mask [n]
// exit 3: the program is refused (the message on stderr), 4: the offsets are not in order
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../csrc/postproc_compile.cpp"

using postproc::Cell;
using postproc::In;
using postproc::List;
using postproc::Opts;
using postproc::Row;

namespace {

constexpr uint64_t kThreads = 256;

std::vector<uint8_t> g_in;
size_t g_at = 0;

void need(size_t n) {
  if (g_at + n > g_in.size()) {
    fprintf(stderr, "postproc_check: short input\n");
    exit(2);
  }
}
uint32_t rd32() {
  need(4);
  uint32_t v;
  memcpy(&v, g_in.data() + g_at, 4);
  g_at += 4;
  return v;
}
uint64_t rd64() {
  need(8);
  uint64_t v;
  memcpy(&v, g_in.data() + g_at, 8);
  g_at += 8;
  return v;
}
std::string rds(uint64_t n) {
  need(n);
  std::string s((const char*)g_in.data() + g_at, n);
  g_at += n;
  return s;
}

template <typename T>
struct Exact {  // a heap block of exactly n elements (none: a null pointer)
  T* p = nullptr;
  uint64_t n = 0;
  explicit Exact(uint64_t n_) : n(n_) { p = n ? (T*)malloc(n * sizeof(T)) : nullptr; }
  Exact(const Exact&) = delete;
  ~Exact() { free(p); }
  void read() {
    need(n * sizeof(T));
    if (n) memcpy(p, g_in.data() + g_at, n * sizeof(T));
    g_at += n * sizeof(T);
  }
  void write() const {
    if (n) fwrite(p, sizeof(T), n, stdout);
  }
};

// a workgroup's staged tables, as stage() of postproc.hip lays them out
struct Staged {
  Exact<uint16_t> tab;
  List single, pair;
  explicit Staged(const postproc::Program& p) : tab((p.single.items.size() + 1 + p.pair.items.size() + 1) * 3) {
    const uint32_t n0 = p.single.items.size() + 1, n1 = p.pair.items.size() + 1;
    for (uint32_t i = 0; i < n0; i++) {
      tab.p[i] = p.single.pa[i];
      tab.p[n0 + i] = p.single.pb[i];
      tab.p[2 * n0 + i] = p.single.ps[i];
    }
    uint16_t* t1 = tab.p + 3 * n0;
    for (uint32_t i = 0; i < n1; i++) {
      t1[i] = p.pair.pa[i];
      t1[n1 + i] = p.pair.pb[i];
      t1[2 * n1 + i] = p.pair.ps[i];
    }
    single = List{tab.p, tab.p + n0, tab.p + 2 * n0, p.single.val.data(), n0 - 1};
    pair = List{t1, t1 + n1, t1 + 2 * n1, p.pair.val.data(), n1 - 1};
  }
};

void put64(uint64_t v) { fwrite(&v, 8, 1, stdout); }

}  // namespace

int main() {
  {
    uint8_t buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, stdin)) > 0) g_in.insert(g_in.end(), buf, buf + k);
  }
  std::vector<postproc::HostStep> steps(rd64());
  for (postproc::HostStep& h : steps) {
    h.kind = rd32();
    h.has_pair_template = rd32() & 1u;
    h.id_a = rd32();
    h.id_b = rd32();
    const uint64_t sl = rd64(), pl = rd64(), nt = rd64();
    h.single = rds(sl);
    h.pair = rds(pl);
    for (uint64_t t = 0; t < nt; t++) {
      const uint64_t len = rd64();
      const uint32_t id = rd32();
      h.specials.emplace_back(rds(len), id);
    }
  }
  postproc::Program prog;
  std::string err;
  const postproc::CompileError ce = postproc::compile(steps, &prog, &err);
  if (ce != postproc::C_OK) {
    fprintf(stderr, "%s\n", err.c_str());
    return ce == postproc::C_CAPACITY ? 3 : 5;
  }

  Opts o{};
  o.truncate = rd32();
  o.strategy = rd32();
  o.truncate_to = rd64();
  const uint32_t padded = rd32();
  o.pad_left = rd32();
  const uint64_t pad_to = rd64();
  o.pad_id = rd32();
  const uint32_t pairs = rd32();
  const uint64_t n_rows = rd64();
  Exact<uint64_t> off(n_rows + 1), pair_off(pairs ? n_rows + 1 : 0);
  off.read();
  pair_off.read();
  Exact<uint8_t> has_pair(pairs == 1 ? n_rows : 0);
  has_pair.read();
  uint64_t n_pair = 0;
  for (uint64_t r = 0; pairs && r < n_rows; r++)
    if ((pairs == 2 || has_pair.p[r]) && pair_off.p[r + 1] > n_pair) n_pair = pair_off.p[r + 1];
  Exact<uint32_t> ids(off.p[n_rows]), pair_ids(n_pair);
  ids.read();
  pair_ids.read();
  In in{ids.p, off.p, pair_ids.p, pairs ? pair_off.p : nullptr, pairs == 1 ? has_pair.p : nullptr, n_rows, ids.n, pair_ids.n};

  // count: a thread per row, the maximum, the scan
  Exact<Row> rows(n_rows);
  Exact<uint64_t> out_off(n_rows + 1);
  uint64_t longest = 0;
  bool bad = false;
  const List single = prog.single.view(), pair = prog.pair.view();
  for (uint64_t r = 0; r < n_rows; r++) {
    out_off.p[r] = postproc::count_row(in, o, single, pair, r, &rows.p[r], &bad);
    if (out_off.p[r] > longest) longest = out_off.p[r];
  }
  if (bad) return 4;
  uint64_t total = 0;
  for (uint64_t r = 0; r <= n_rows; r++) {
    const uint64_t len = r < n_rows ? out_off.p[r] : 0;
    out_off.p[r] = total;
    total += len;
  }

  put64(prog.single.items.size());
  put64(prog.pair.items.size());
  if (!padded) {
    Exact<uint32_t> out(total);
    // a workgroup takes a run of kRun consecutive tiles (the kernel: the tiles over its grid), stages the tables,
    // finds the rows of the run's first and last cell, and its threads walk up from there
    constexpr uint64_t kRun = 3;
    for (uint64_t c_first = 0; c_first < total; c_first += kRun * kThreads) {
      const Staged st(prog);
      const uint64_t c_last = (c_first + kRun * kThreads < total ? c_first + kRun * kThreads : total) - 1;
      const uint64_t r_lo = postproc::find_row(out_off.p, 0, n_rows - 1, c_first);
      const uint64_t r_hi = postproc::find_row(out_off.p, 0, n_rows - 1, c_last);
      for (uint64_t t = 0; t < kThreads; t++) {
        uint64_t r = r_lo;
        for (uint64_t c = c_first + t; c <= c_last; c += kThreads) {
          r = postproc::find_row(out_off.p, r, r_hi, c);
          const List& l = postproc::row_has_pair(in, r) ? st.pair : st.single;
          const Cell cell = postproc::cell_of(l, rows.p[r].na, rows.p[r].nb, c - out_off.p[r]);
          out.p[c] = postproc::cell_id(in, r, cell);
        }
      }
    }
    put64(total);
    put64(longest);
    out_off.write();
    out.write();
    return 0;
  }
  const uint64_t width = longest > pad_to ? longest : pad_to, cells = n_rows * width;
  Exact<uint32_t> row_len(n_rows), m_ids(cells), m_attn(cells), m_type(cells), m_special(cells);
  for (uint64_t r = 0; r < n_rows; r++) row_len.p[r] = (uint32_t)(out_off.p[r + 1] - out_off.p[r]);
  for (uint64_t c0 = 0; c0 < cells; c0 += kThreads) {
    const Staged st(prog);
    for (uint64_t c = c0; c < cells && c < c0 + kThreads; c++) {
      const uint64_t r = c / width, col = c - r * width, len = out_off.p[r + 1] - out_off.p[r];
      const uint64_t j = postproc::matrix_cell(width, len, o.pad_left != 0, col);
      uint32_t id = o.pad_id, attention = 0, type = 0, special = 1;
      if (j != postproc::kNoCell) {
        const List& l = postproc::row_has_pair(in, r) ? st.pair : st.single;
        const Cell cell = postproc::cell_of(l, rows.p[r].na, rows.p[r].nb, j);
        id = postproc::cell_id(in, r, cell);
        attention = 1;
        type = cell.kind == postproc::IT_B;
        special = cell.kind == postproc::IT_SPECIAL;
      }
      m_ids.p[c] = id;
      m_attn.p[c] = attention;
      m_type.p[c] = type;
      m_special.p[c] = special;
    }
  }
  put64(cells);
  put64(width);
  row_len.write();
  m_ids.write();
  m_attn.write();
  m_type.write();
  m_special.write();
  return 0;
}
