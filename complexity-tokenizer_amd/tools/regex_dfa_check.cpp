// CPU driver of csrc/regex_dfa.{h,cpp} (a `split` pattern compiled to a DFA) and of the rules that run
// it (csrc/pretok_hd.h dfa_len, dfa_walk) for tests/test_regex_dfa_cpu.py, which compares with the
// `regex` module.
// Build: g++ -O1 -std=c++17 -fsanitize=address,undefined regex_dfa_check.cpp -o regex_dfa_check
// regex_dfa_check --plan PATTERN prints "gate symbols states nfa cyclic longest" and, on a second
//   line, why the pattern is refused (gate: 1 literal, 2 class atom, 3 refused, 4 DFA; PATTERN is one
//   the Rust crate compiles).
// regex_dfa_check [--cap R]
//   stdin:  u64 pattern length, the pattern; u64 n, u64 off[n + 1] and off[n] bytes: n texts
//   stdout: u32 len[off[n]] (the match that starts at each byte, 0: none), u8 mark[off[n]] (the
//           leftmost non-overlapping matches: kInMatch | kMatchStart), u32 over (the lowest start
//           whose run passes R code points, 0xFFFFFFFF: none)
// Every text is one word.  The matches' ends go through the prefix max the way the kernels take it:
// per tile of kTile bytes, a carry over the tiles, then byte by byte inside the tile; the buffers
// are exactly as long as the batch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../csrc/regex_dfa.cpp"
#include "../csrc/pretok_prog.h"

using namespace pretok;

constexpr uint64_t kTile = 1024;  // pretok_internal.h kWaveTile

static bool read_all(void* p, size_t n) { return !n || fread(p, 1, n, stdin) == n; }

int main(int argc, char** argv) {
  if (argc > 2 && !strcmp(argv[1], "--plan")) {
    HostStep h;
    std::string why;
    const int gate = (int)plan_split(argv[2], &h, &why);
    printf("%d %u %u %u %d %llu\n%s\n", gate, h.dfa.n_symbols, h.dfa.n_states, h.dfa.n_nfa, h.dfa.cyclic ? 1 : 0,
           (unsigned long long)h.dfa.longest, why.c_str());
    return 0;
  }
  uint32_t cap = 0xFFFFFFFFu;
  if (argc > 2 && !strcmp(argv[1], "--cap")) cap = (uint32_t)strtoul(argv[2], nullptr, 10);
  const Tables T{ct_cls_stage1, ct_cls_stage2, pt_nd_lo, pt_nd_hi, PT_N_ND};
  uint64_t plen = 0;
  if (!read_all(&plen, 8)) return 2;
  std::string pattern(plen, '\0');
  if (!read_all(&pattern[0], plen)) return 2;
  HostStep h;
  h.kind = K_SPLIT;
  h.mode = M_DFA;
  const std::string why = regex_dfa::compile(pattern, &h.dfa);
  if (!why.empty()) {
    fprintf(stderr, "refused: %s\n", why.c_str());
    return 7;
  }
  const StepBlob blob = step_blob(h);
  const Step st = step_view(h, blob, (const uint8_t*)blob.bytes.data(), cap);
  uint64_t nd = 0;
  if (!read_all(&nd, 8)) return 2;
  std::vector<uint64_t> off(nd + 1);
  if (!read_all(off.data(), (nd + 1) * 8)) return 2;
  const uint64_t n = off[nd];
  std::vector<uint8_t> text(n ? n : 1);
  if (!read_all(text.data(), n)) return 2;
  std::vector<uint64_t> inw((n + 63) / 64 + 1, 0), beg((n + 63) / 64 + 1, 0);
  for (uint64_t p = 0; p < n; p++) inw[p >> 6] |= 1ull << (p & 63);
  for (uint64_t d = 0; d < nd; d++)
    if (off[d] < off[d + 1]) beg[off[d] >> 6] |= 1ull << (off[d] & 63);
  const Ctx x{text.data(), n, inw.data(), beg.data()};

  std::vector<uint32_t> len(n ? n : 1, 0);
  std::vector<uint8_t> mark(n ? n : 1, 0);
  uint32_t over = 0xFFFFFFFFu;
  for (uint64_t p = 0; p < n; p++) {
    bool ov;
    len[p] = dfa_len(T, st.dfa, st.dfa.trans, x, p, &ov);
    if (len[p] > n - p) return 3;
    if (ov) over = std::min<uint32_t>(over, (uint32_t)p);
  }
  const uint64_t nt = (n + kTile - 1) / kTile;
  std::vector<uint32_t> tmax(nt + 1, 0), carry(nt + 1, 0);
  for (uint64_t t = 0; t < nt; t++)
    for (uint64_t p = t * kTile; p < std::min(n, (t + 1) * kTile); p++)
      if (len[p]) tmax[t] = std::max<uint32_t>(tmax[t], (uint32_t)p + len[p]);
  for (uint64_t t = 1; t < nt; t++) carry[t] = std::max(carry[t - 1], tmax[t - 1]);
  for (uint64_t t = 0; t < nt; t++) {
    uint32_t reach = carry[t];
    for (uint64_t p = t * kTile; p < std::min(n, (t + 1) * kTile); p++) {
      if (len[p] && reach <= p) dfa_walk(len.data(), n, p, mark.data());
      if (len[p]) reach = std::max<uint32_t>(reach, (uint32_t)p + len[p]);
    }
  }
  fwrite(len.data(), 4, n, stdout);
  fwrite(mark.data(), 1, n, stdout);
  fwrite(&over, 4, 1, stdout);
  return 0;
}
