// CPU driver of csrc/pretok_hd.h (the PreTokenizer's rules behind pretok.hip) for
// tests/test_pretok_cpu.py, which compares its output with a restatement in plain Python.
// Build: g++ -O1 -std=c++17 -fsanitize=address,undefined pretok_check.cpp -o pretok_check
// stdin:  u64 n_steps, per step u32 kind, u32 flags, u32 cp, u64 a_len, a (the steps of
//         include/ctok_pretokenizer.h, a split's flags with CTOK_PRETOK_REGEX or without; a pattern the
//         Rust crate rejects comes with kind | 0x100);
//         then u64 n, u64 off[n + 1] and off[n] bytes: n texts
// stdout: u64 n_words, u64 n_bytes, u64 text_word[n + 1], u64 word_off[n_words + 1], the bytes
// pretok_check --classify PATTERN prints 1 (literal), 2 (class atom) or 3 (unsupported).
// Every step runs the way the kernels run it: bitmap word by bitmap word for the splitters (the
// script carry from the words before), count per bitmap word, sums and write into buffers of exactly
// the counted size for the rewriters and the final gather.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../csrc/gen/pretok_data.h"
#include "../csrc/gen/unicode_data.h"
#include "../csrc/regex_dfa.cpp"
#include "../csrc/pretok_hd.h"
#include "../csrc/pretok_prog.h"

using namespace pretok;

static bool read_all(void* p, size_t n) { return !n || fread(p, 1, n, stdin) == n; }

struct Batch {
  std::vector<uint8_t> text;  // exactly the bytes (one spare when empty: data() stays valid)
  std::vector<uint64_t> inw, beg;
  uint64_t n = 0;
  Ctx ctx() const { return Ctx{text.data(), n, inw.data(), beg.data()}; }
  uint64_t words64() const { return (n + 63) / 64; }
};

struct Words {
  std::vector<uint64_t> text_word, word_off;
  std::vector<uint8_t> bytes;
};

// (the blob must outlive the Step)
static Step dev_step(const HostStep& h, const StepBlob& blob) {
  return step_view(h, blob, (const uint8_t*)blob.bytes.data(), 0xFFFFFFFFu);
}

static void split_step(const Tables& T, const HostStep& h, Batch& b) {
  const StepBlob blob = step_blob(h);
  Step st = dev_step(h, blob);
  const Ctx x = b.ctx();
  const uint64_t n = b.n, nw = b.words64();
  std::vector<uint8_t> cand(n + 1, 0), mark(n + 1, 0), whit;
  std::vector<uint64_t> wpos(nw + 1, 0);
  if (h.kind == K_SPLIT && h.mode == M_LITERAL) {
    for (uint64_t p = 0; p < n; p++) cand[p] = lit_cand(st, x, p);
    st.cand = cand.data();
    for (uint64_t p = 0; p < n; p++) lit_chain(st, n, p, mark.data());
    st.mark = mark.data();
  }
  std::vector<uint32_t> len;
  if (h.kind == K_SPLIT && h.mode == M_DFA) {
    // every start's match, then the chain heads by the running maximum of the matches' ends
    len.assign(n + 1, 0);
    for (uint64_t p = 0; p < n; p++) {
      bool over;
      len[p] = dfa_len(T, st.dfa, st.dfa.trans, x, p, &over);
    }
    uint64_t reach = 0;
    for (uint64_t p = 0; p < n; p++) {
      if (len[p] && reach <= p) dfa_walk(len.data(), n, p, mark.data());
      if (len[p]) reach = std::max<uint64_t>(reach, p + len[p]);
    }
    st.mark = mark.data();
  }
  if (h.kind == K_SPLIT && h.mode != M_IDENTITY && (h.flags & 15u) == B_REMOVED) {
    for (uint64_t j = 0; j < nw; j++) wpos[j + 1] = wpos[j] + __builtin_popcountll(b.beg[j]);
    st.wpos = wpos.data();
    whit.assign(wpos[nw] + 1, 0);
    for (uint64_t p = 0; p < n; p++) {
      if (!in_word(x, p) || unit_lead(x, p) != p) continue;
      uint32_t l;
      if (split_in(T, st, x, p, cp_at(x, p, &l))) whit[word_of(st, x, p)] = 1;
    }
    st.whit = whit.data();
  }
  std::vector<uint64_t> inw(nw + 1, 0), beg(nw + 1, 0);
  uint32_t carry = 0;  // UnicodeScripts: the last non-zero value of the words before
  for (uint64_t j = 0; j < nw; j++) {
    uint32_t sv = carry;
    for (uint64_t p = j * 64; p < std::min(n, j * 64 + 64); p++) {
      bool in, bg;
      split_bits(T, st, x, p, sv, &in, &bg);
      if (in) inw[j] |= 1ull << (p & 63);
      if (bg) beg[j] |= 1ull << (p & 63);
      if (h.kind == K_SCRIPTS) {
        const uint32_t v = script_val(x, p);
        if (v) sv = v;
      }
    }
    carry = sv;
  }
  b.inw.swap(inw);
  b.beg.swap(beg);
}

// false: the count and the write disagree
static bool rewrite_step(const Tables& T, const HostStep& h, Batch& b) {
  const StepBlob blob = step_blob(h);
  const Step st = dev_step(h, blob);
  const Ctx x = b.ctx();
  const uint64_t n = b.n, nw = b.words64();
  std::vector<uint64_t> pos(nw + 1, 0);
  uint8_t unit[kMaxUnit];
  bool bg;
  for (uint64_t j = 0; j < nw; j++) {
    uint64_t c = 0;
    for (uint64_t p = j * 64; p < std::min(n, j * 64 + 64); p++) c += rw_unit(T, st, x, p, unit, &bg);
    pos[j + 1] = pos[j] + c;
  }
  Batch out;
  out.n = pos[nw];
  out.text.assign(out.n ? out.n : 1, 0xEE);
  out.inw.assign(out.words64() + 1, 0);
  out.beg.assign(out.words64() + 1, 0);
  for (uint64_t j = 0; j < nw; j++) {
    uint64_t o = pos[j];
    for (uint64_t p = j * 64; p < std::min(n, j * 64 + 64); p++) {
      const uint32_t l = rw_unit(T, st, x, p, unit, &bg);
      if (l > kMaxUnit || o + l > out.n) return false;
      memcpy(out.text.data() + o, unit, l);
      if (l && bg) out.beg[o >> 6] |= 1ull << (o & 63);
      o += l;
    }
    if (o != pos[j + 1]) return false;
  }
  for (uint64_t p = 0; p < out.n; p++) out.inw[p >> 6] |= 1ull << (p & 63);
  b = out;
  return true;
}

static bool run(const Tables& T, const std::vector<HostStep>& prog, const std::vector<uint8_t>& text,
                const std::vector<uint64_t>& off, Words& w);

// the words every empty text gets
static bool empty_words(const Tables& T, const std::vector<HostStep>& prog, Words& w) {
  size_t at = 0;
  w = Words{{0, 0}, {0}, {}};
  const EmptyFate f = empty_fate(prog, &at);
  if (f == E_NOTHING) return true;
  if (f == E_EMPTY_WORD) {
    w.text_word = {0, 1};
    w.word_off = {0, 0};
    return true;
  }
  std::vector<HostStep> sub(prog.begin() + at, prog.end());
  sub[0].flags &= ~1u;  // (Metaspace with a prefix over "" is Metaspace without one over the replacement)
  std::vector<uint8_t> text(sub[0].cp_u8.begin(), sub[0].cp_u8.end());
  return run(T, sub, text, {0, text.size()}, w);
}

static bool run(const Tables& T, const std::vector<HostStep>& prog, const std::vector<uint8_t>& text,
                const std::vector<uint64_t>& off, Words& w) {
  const uint64_t nd = off.size() - 1;
  Batch b;
  b.n = off[nd];
  b.text.assign(text.begin(), text.begin() + b.n);
  if (b.text.empty()) b.text.resize(1);
  b.inw.assign(b.words64() + 1, 0);
  b.beg.assign(b.words64() + 1, 0);
  for (uint64_t p = 0; p < b.n; p++) b.inw[p >> 6] |= 1ull << (p & 63);
  for (uint64_t d = 0; d < nd; d++)
    if (off[d] < off[d + 1]) b.beg[off[d] >> 6] |= 1ull << (off[d] & 63);
  // a text's first byte in the current buffer: a rewriter moves it
  std::vector<uint64_t> cur_off(off);
  for (const HostStep& h : prog) {
    if (!rewrites(h.kind)) {
      split_step(T, h, b);
      continue;
    }
    // (a text's new offset: the output bytes of the input bytes before it)
    const StepBlob blob = step_blob(h);
    const Step st = dev_step(h, blob);
    const Ctx x = b.ctx();
    std::vector<uint64_t> before(b.n + 1, 0);
    uint8_t unit[kMaxUnit];
    bool bg;
    for (uint64_t p = 0; p < b.n; p++) before[p + 1] = before[p] + rw_unit(T, st, x, p, unit, &bg);
    for (uint64_t& o : cur_off) o = before[o];
    if (!rewrite_step(T, h, b)) return false;
  }
  Words ew;
  bool has_empty = false;
  for (uint64_t d = 0; d < nd; d++) has_empty = has_empty || off[d] == off[d + 1];
  if (has_empty && !empty_words(T, prog, ew)) return false;
  // the gather: counts per bitmap word, sums, write into exactly the counted size
  const uint64_t nw = b.words64();
  std::vector<uint64_t> posb(nw + 1, 0), posw(nw + 1, 0);
  for (uint64_t j = 0; j < nw; j++) {
    posb[j + 1] = posb[j] + __builtin_popcountll(b.inw[j]);
    posw[j + 1] = posw[j] + __builtin_popcountll(b.beg[j]);
  }
  std::vector<uint64_t> ex(nd + 1, 0);
  for (uint64_t d = 0; d < nd; d++) ex[d + 1] = ex[d] + (has_empty && off[d] == off[d + 1] ? 1 : 0);
  const uint64_t ewn = has_empty ? ew.word_off.size() - 1 : 0, ebn = has_empty ? ew.bytes.size() : 0;
  const uint64_t n_words = posw[nw] + ex[nd] * ewn, n_bytes = posb[nw] + ex[nd] * ebn;
  w.bytes.assign(n_bytes ? n_bytes : 1, 0xEE);
  w.word_off.assign(n_words + 1, ~0ull);
  w.text_word.assign(nd + 1, 0);
  uint64_t d = 0;
  for (uint64_t p = 0; p < b.n; p++) {
    while (d + 1 < nd && p >= cur_off[d + 1]) d++;
    if (!bit(b.inw.data(), p)) continue;
    const uint64_t below = (1ull << (p & 63)) - 1;
    const uint64_t ob = posb[p >> 6] + __builtin_popcountll(b.inw[p >> 6] & below) + ex[d] * ebn;
    if (ob >= n_bytes) return false;
    w.bytes[ob] = b.text[p];
    if (bit(b.beg.data(), p)) {
      const uint64_t wi = posw[p >> 6] + __builtin_popcountll(b.beg[p >> 6] & below) + ex[d] * ewn;
      if (wi >= n_words) return false;
      w.word_off[wi] = ob;
    }
  }
  for (uint64_t t = 0; t <= nd; t++) {
    const uint64_t o = cur_off[t], below = (1ull << (o & 63)) - 1;
    const uint64_t wb = o < b.n ? posw[o >> 6] + __builtin_popcountll(b.beg[o >> 6] & below) : posw[nw];
    const uint64_t bb = o < b.n ? posb[o >> 6] + __builtin_popcountll(b.inw[o >> 6] & below) : posb[nw];
    w.text_word[t] = wb + ex[t] * ewn;
    if (t < nd && ex[t + 1] != ex[t]) {
      for (uint64_t k = 0; k < ewn; k++) w.word_off[w.text_word[t] + k] = bb + ex[t] * ebn + ew.word_off[k];
      if (ebn) memcpy(w.bytes.data() + bb + ex[t] * ebn, ew.bytes.data(), ebn);
    }
  }
  w.word_off[n_words] = n_bytes;
  w.bytes.resize(n_bytes);
  return true;
}

int main(int argc, char** argv) {
  if (argc > 2 && !strcmp(argv[1], "--classify")) {
    printf("%d\n", (int)classify_split(argv[2], nullptr));
    return 0;
  }
  const Tables T{ct_cls_stage1, ct_cls_stage2, pt_nd_lo, pt_nd_hi, PT_N_ND};
  uint64_t n_steps = 0;
  if (!read_all(&n_steps, 8)) return 2;
  std::vector<HostStep> prog(n_steps);
  for (uint64_t i = 0; i < n_steps; i++) {
    uint32_t kfc[3];
    uint64_t len;
    if (!read_all(kfc, 12) || !read_all(&len, 8)) return 2;
    std::string a(len, '\0');
    if (!read_all(&a[0], len)) return 2;
    bool unsupported;
    if (!make_step(kfc[0] & 0xFFu, kfc[1], a, kfc[2], (kfc[0] & 0x100u) != 0, &prog[i], &unsupported).empty()) return unsupported ? 7 : 5;
  }
  uint64_t n = 0;
  if (!read_all(&n, 8)) return 2;
  std::vector<uint64_t> off(n + 1);
  if (!read_all(off.data(), (n + 1) * 8)) return 2;
  std::vector<uint8_t> text(off[n] ? off[n] : 1);
  if (!read_all(text.data(), off[n])) return 2;
  Words w;
  if (!run(T, prog, text, off, w)) return 3;
  const uint64_t head[2] = {w.word_off.size() - 1, w.bytes.size()};
  fwrite(head, 8, 2, stdout);
  fwrite(w.text_word.data(), 8, w.text_word.size(), stdout);
  fwrite(w.word_off.data(), 8, w.word_off.size(), stdout);
  fwrite(w.bytes.data(), 1, w.bytes.size(), stdout);
  return 0;
}
