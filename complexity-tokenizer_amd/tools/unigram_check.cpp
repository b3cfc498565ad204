// CPU driver of csrc/unigram_hd.h (what unigram.hip's kernels share): reads one job from stdin, does
// it the way the kernels' threads do, writes the result to stdout.  tests/test_unigram_cpu.py makes the
// jobs and compares with the Python restatement.  All integers are little-endian u64, scores f64.
//   job 1  encode: patterns (bytes, symbol), scores by symbol, the fallback (symbol, score), the
//          window (chars) and texts -> per text its ids: the table lookup at every char start
//          (matches), a Viterbi step per end over the candidates in descending start order (the
//          opposite of the reference's, so only takes() decides) and the model's back walk
//   job 2  Metaspace: documents -> sentence offsets and bytes, span by span (meta_range), a
//          measuring pass, the two prefix sums and a writing pass
//   job 3  substrings: sentences and max chars -> every (start, end) that k_sub_count would add
// Build: g++ -O2 -std=c++17 unigram_check.cpp -o unigram_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../csrc/unigram_hd.h"

static std::vector<uint8_t> in;
static size_t at = 0;
static std::vector<uint8_t> out;

static uint64_t get() {
  uint64_t v = 0;
  if (at + 8 > in.size()) exit(3);
  memcpy(&v, &in[at], 8);
  at += 8;
  return v;
}
static double getf() {
  const uint64_t v = get();
  double d;
  memcpy(&d, &v, 8);
  return d;
}
static std::string gets_(uint64_t n) {
  if (at + n > in.size()) exit(3);
  std::string s((const char*)&in[at], n);
  at += n;
  return s;
}
static void put(uint64_t v) {
  const uint8_t* p = (const uint8_t*)&v;
  out.insert(out.end(), p, p + 8);
}

struct Texts {
  std::vector<uint64_t> off;
  std::string bytes;  // 16 spare bytes behind them
  uint64_t n() const { return off.size() - 1; }
  uint64_t nb() const { return off.back(); }
  const uint8_t* p() const { return (const uint8_t*)bytes.data(); }
};
static Texts get_texts() {
  Texts t;
  const uint64_t n = get();
  for (uint64_t i = 0; i <= n; i++) t.off.push_back(get());
  t.bytes = gets_(t.off[n]) + std::string(16, '\0');
  return t;
}
static std::vector<uint32_t> start_bits(const Texts& t) {
  std::vector<uint32_t> bits(t.nb() / 32 + 2, 0);
  for (uint64_t k = 0; k < t.n(); k++)
    if (t.off[k] < t.off[k + 1]) bits[t.off[k] >> 5] |= 1u << (t.off[k] & 31);
  return bits;
}

static int job_encode() {
  const uint64_t n_pat = get();
  std::vector<std::string> strs(n_pat);
  std::vector<wptab::Pattern> pats;
  for (uint64_t i = 0; i < n_pat; i++) {
    strs[i] = gets_(get());
    const uint32_t sym = (uint32_t)get();
    pats.push_back(wptab::Pattern{(const uint8_t*)strs[i].data(), (uint32_t)strs[i].size(), 0, sym});
  }
  std::vector<double> score(get());
  for (auto& s : score) s = getf();
  const uint32_t fb_sym = (uint32_t)get();
  const double fb_score = getf();
  const uint32_t wl = (uint32_t)get(), wv = (uint32_t)get();
  const Texts t = get_texts();
  wptab::Built b;
  if (wptab::build(pats, &b) != wptab::kOk) return 4;
  const wptab::View v = b.view();
  const std::vector<uint32_t> bits = start_bits(t);
  const uint64_t nb = t.nb();
  // the char index of every byte and the lattice, a "thread" per byte
  std::vector<uint32_t> cidx(nb + 1, 0);
  for (uint64_t p = 0; p < nb; p++) cidx[p + 1] = cidx[p] + uni::is_lead(t.p()[p]);
  const uint32_t nc = cidx[nb];
  std::vector<uint32_t> lat((size_t)wl * nc + 1, 0xDEADBEEFu);
  for (uint64_t p = 0; p < nb; p++) {
    if (!uni::is_lead(t.p()[p])) continue;
    const uint32_t c = cidx[p];
    uint32_t next = 0;
    uni::matches(v, t.p(), nb, bits.data(), p, wl, [&](uint32_t j, uint32_t sym) {
      for (; next < j; next++) lat[(size_t)next * nc + c] = uni::kNone;
      lat[(size_t)j * nc + c] = sym;
      next = j + 1;
    });
    for (; next < wl; next++) lat[(size_t)next * nc + c] = uni::kNone;
  }
  for (uint64_t k = 0; k < t.n(); k++) {
    const uint32_t c0 = cidx[t.off[k]], c1 = cidx[t.off[k + 1]], n = c1 - c0;
    std::vector<double> best(n + 1, -__builtin_inf());
    std::vector<uint32_t> blen(n + 1, 0), bsym(n + 1, uni::kNone);
    best[0] = 0.0;
    for (uint32_t e = 1; e <= n; e++) {
      double t_sum = -__builtin_inf();
      uint32_t t_j = 0, t_sym = uni::kNone;
      const uint32_t w = wv < e ? wv : e;
      for (uint32_t j = 0; j < w; j++) {
        const uint32_t st = e - j - 1;
        uint32_t sym = j < wl ? lat[(size_t)j * nc + c0 + st] : uni::kNone;
        double sc;
        if (sym != uni::kNone) sc = score[sym];
        else if (j == 0) { sc = fb_score; sym = fb_sym; }
        else continue;
        const double sum = best[st] + sc;
        if (uni::takes(sum, j, t_sum, t_j)) {
          t_sum = sum;
          t_j = j;
          t_sym = sym;
        }
      }
      if (t_sum > -__builtin_inf()) {
        best[e] = t_sum;
        blen[e] = t_j + 1;
        bsym[e] = t_sym;
      }
    }
    std::vector<uint64_t> ids;
    for (uint32_t pos = n; pos > 0;) {
      if (!blen[pos]) {
        ids.push_back(0);
        break;
      }
      ids.push_back(bsym[pos]);
      pos -= blen[pos];
    }
    put(ids.size());
    for (size_t i = ids.size(); i-- > 0;) put(ids[i]);
  }
  return 0;
}

static int job_meta() {
  const Texts t = get_texts();
  const uint64_t nb = t.nb(), n_spans = nb / uni::kSpan + 1;
  std::vector<uint64_t> len(n_spans + 1, 0), ns(n_spans + 1, 0);
  for (uint64_t i = 0; i < n_spans; i++) {
    const uint64_t b0 = i * uni::kSpan, b1 = b0 + uni::kSpan < nb + 1 ? b0 + uni::kSpan : nb + 1;
    uni::meta_range(t.p(), nb, t.off.data(), t.n(), b0, b1, nullptr, 0, nullptr, &len[i], &ns[i]);
  }
  uint64_t a = 0, b = 0;
  for (uint64_t i = 0; i <= n_spans; i++) {  // exclusive, the totals last
    const uint64_t l = len[i], s = ns[i];
    len[i] = a;
    ns[i] = b;
    a += l;
    b += s;
  }
  std::vector<uint8_t> o(len[n_spans] + 1, 0xEE);
  std::vector<uint64_t> so(ns[n_spans] + 1, ~0ull);
  for (uint64_t i = 0; i < n_spans; i++) {
    const uint64_t b0 = i * uni::kSpan, b1 = b0 + uni::kSpan < nb + 1 ? b0 + uni::kSpan : nb + 1;
    uint64_t x, y;
    uni::meta_range(t.p(), nb, t.off.data(), t.n(), b0, b1, o.data() + len[i], len[i], so.data() + ns[i], &x, &y);
    if (x != len[i + 1] - len[i] || y != ns[i + 1] - ns[i]) return 5;
  }
  so[ns[n_spans]] = len[n_spans];
  put(ns[n_spans]);
  for (uint64_t v : so) put(v);
  out.insert(out.end(), o.begin(), o.begin() + len[n_spans]);
  return 0;
}

static int job_substrings() {
  const uint64_t max_chars = get();
  const Texts t = get_texts();
  const std::vector<uint32_t> bits = start_bits(t);
  std::vector<uint64_t> pairs;
  for (uint64_t p = 0; p < t.nb(); p++) {
    if (!uni::is_lead(t.p()[p])) continue;
    uni::substrings(t.p(), t.nb(), bits.data(), p, max_chars, [&](uint64_t e) {
      pairs.push_back(p);
      pairs.push_back(e);
    });
  }
  put(pairs.size() / 2);
  for (uint64_t v : pairs) put(v);
  return 0;
}

int main() {
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, stdin)) > 0) in.insert(in.end(), buf, buf + n);
  const uint64_t job = get();
  const int rc = job == 1 ? job_encode() : job == 2 ? job_meta() : job == 3 ? job_substrings() : 2;
  if (rc) return rc;
  fwrite(out.data(), 1, out.size(), stdout);
  return 0;
}
