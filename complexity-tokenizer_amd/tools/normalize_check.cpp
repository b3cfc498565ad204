// CPU driver of csrc/normalize_hd.h (the Normalizer's steps behind normalize.hip) for
// tests/test_normalize_cpu.py, which compares its output with a restatement in plain Python.
// Build: g++ -O1 -std=c++17 -fsanitize=address,undefined normalize_check.cpp -o normalize_check
// stdin:  u64 n_steps, per step u32 kind, u32 flags, u64 a_len, u64 b_len, a, b (the steps of
//         include/ctok_normalizer.h); then u64 n, u64 off[n + 1] and off[n] bytes: n texts
// stdout: u64 out_off[n + 1], then out_off[n] bytes
// With --steps the number of inner-loop steps taken (NZ_STEP in the header: ordering, composition,
// chain walks, trimming) goes to stderr.
// Every primitive step runs the way the kernels run it: span by span a count, the sums, span by
// span the write into a buffer of exactly the counted size, text by text the new offsets.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define NZ_COUNT_STEPS
uint64_t nz_steps = 0;

#include "../csrc/gen/lowercase_data.h"
#include "../csrc/gen/normalize_data.h"
#include "../csrc/lowercase_hd.h"
#include "../csrc/normalize_hd.h"
#include "../csrc/normalize_prog.h"

using namespace normalize;

static bool read_all(void* p, size_t n) { return !n || fread(p, 1, n, stdin) == n; }

struct Batch {
  std::vector<uint8_t> text;  // exactly the batch's bytes (one spare when empty: data() stays valid)
  std::vector<uint64_t> off;
  uint64_t bytes() const { return off.back(); }
  uint64_t docs() const { return off.size() - 1; }
};

static void lower_step(const Batch& in, Batch& out) {
  const lowercase::Tables T{lc_map_from, lc_map_to, LC_N_MAP, lc_cased, LC_N_CASED_RANGES, lc_ignorable,
                            LC_N_IGNORABLE_RANGES};
  out.text.clear();
  out.off.assign(1, 0);
  for (uint64_t d = 0; d < in.docs(); d++) {
    const uint64_t lo = in.off[d], hi = in.off[d + 1];
    for (uint64_t p = lo; p < hi; p++) {
      if (!lowercase::is_start(in.text.data(), lo, hi, p)) continue;
      uint8_t buf[4];
      uint32_t in_len;
      bool same;
      const uint32_t len = lowercase::lower_at(T, in.text.data(), lo, hi, p, &in_len, &same, buf);
      out.text.insert(out.text.end(), buf, buf + len);
    }
    out.off.push_back(out.text.size());
  }
  if (out.text.empty()) out.text.resize(1);
}

// false: the count and the write disagree
static bool prim_step(const Tables& T, const PrimStep& ps, const Batch& in, Batch& out) {
  const uint64_t nb = in.bytes(), nd = in.docs(), n_spans = (nb + kSpan - 1) / kSpan;
  const uint8_t* t = in.text.data();
  Step st{};
  st.kind = ps.kind;
  st.a = (const uint8_t*)ps.a.data();
  st.a_len = (uint32_t)ps.a.size();
  st.b = (const uint8_t*)ps.b.data();
  st.b_len = (uint32_t)ps.b.size();
  std::vector<uint64_t> trim(2 * nd + 1);
  std::vector<uint8_t> cand(nb + 1), taken(nb + 1, 0);
  if (ps.kind == P_STRIP) {
    for (uint64_t d = 0; d < nd; d++) trim_bounds(t, in.off[d], in.off[d + 1], &trim[2 * d], &trim[2 * d + 1]);
    st.trim = trim.data();
  }
  if (ps.kind == P_REPLACE) {
    for (uint64_t i = 0; i < n_spans; i++)
      cand_run(st, t, in.off.data(), nd, i * kSpan, std::min<uint64_t>(nb, (i + 1) * kSpan), cand.data());
    st.cand = cand.data();
    for (uint64_t i = 0; i < n_spans; i++)
      chain_run(st, in.off.data(), nd, i * kSpan, std::min<uint64_t>(nb, (i + 1) * kSpan), taken.data());
    st.taken = taken.data();
  }
  std::vector<uint64_t> pos(n_spans + 1, 0);
  bool changed = pre_len(st) + post_len(st) != 0;  // (constants around every text, an empty one too)
  for (uint64_t i = 0; i < n_spans; i++)
    pos[i + 1] = pos[i] + span_run(T, st, t, in.off.data(), nd, i * kSpan, std::min<uint64_t>(nb, (i + 1) * kSpan),
                                   nullptr, &changed);
  const uint64_t total = pos[n_spans] + nd * (pre_len(st) + post_len(st));
  out.text.assign(total ? total : 1, 0xEE);
  out.off.assign(nd + 1, 0);
  for (uint64_t i = 0; i < n_spans; i++) {
    bool ch = false;
    const uint64_t n = span_run(T, st, t, in.off.data(), nd, i * kSpan, std::min<uint64_t>(nb, (i + 1) * kSpan),
                                out.text.data() + pos[i], &ch);
    if (n != pos[i + 1] - pos[i]) return false;
  }
  for (uint64_t d = 0; d <= nd; d++)
    out.off[d] = off_run(T, st, t, nb, in.off.data(), nd, n_spans, pos.data(), d, out.text.data());
  if (out.off[nd] != total) return false;
  if (!changed && (total != nb || memcmp(out.text.data(), t, nb))) return false;  // (an unchanged step is not copied)
  return true;
}

int main(int argc, char** argv) {
  const Tables T{nz_run_index, nz_run_start, nz_run_val, NZ_N_RUNS, NZ_N_INDEXED, NZ_RUN_SHIFT,
                 nz_d_cp, nz_d_loc, NZ_N_D, nz_k_cp, nz_k_loc, NZ_N_K, nz_kr_first, nz_kr_count, nz_kr_to, NZ_N_KR,
                 nz_pool, nz_comp_key, nz_comp_to, NZ_N_COMP};
  uint64_t n_steps = 0;
  if (!read_all(&n_steps, 8)) return 2;
  std::vector<PrimStep> prog;
  for (uint64_t i = 0; i < n_steps; i++) {
    uint32_t kf[2];
    uint64_t len[2];
    if (!read_all(kf, 8) || !read_all(len, 16)) return 2;
    std::string a(len[0], '\0'), b(len[1], '\0');
    if (!read_all(&a[0], len[0]) || !read_all(&b[0], len[1])) return 2;
    if (expand(kf[0], kf[1], a, b, prog)) return 5;
  }
  if (prog.size() > CTOK_NORM_MAX_STEPS) return 6;
  uint64_t n = 0;
  if (!read_all(&n, 8)) return 2;
  Batch cur, next;
  cur.off.resize(n + 1);
  if (!read_all(cur.off.data(), (n + 1) * 8)) return 2;
  cur.text.resize(cur.bytes() ? cur.bytes() : 1);
  if (!read_all(cur.text.data(), cur.bytes())) return 2;
  for (const PrimStep& ps : prog) {
    if (!n) break;
    if (ps.kind == P_LOWER) lower_step(cur, next);
    else if (!prim_step(T, ps, cur, next)) return 3;
    std::swap(cur, next);
  }
  if (argc > 1 && !strcmp(argv[1], "--steps")) fprintf(stderr, "%llu\n", (unsigned long long)nz_steps);
  fwrite(cur.off.data(), 8, n + 1, stdout);
  fwrite(cur.text.data(), 1, cur.bytes(), stdout);
  return 0;
}
