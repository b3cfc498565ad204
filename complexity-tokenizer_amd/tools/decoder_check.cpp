// CPU check of csrc/decoder_hd.h, the Decoder's rules behind csrc/decoder.hip: runs a program over a
// packed batch the way the kernels' threads do -- a thread per unit in workgroups of 256, the
// preparation, the count per workgroup, the scan, the write -- with every buffer exactly as long as
// what was counted, so that the address sanitizer sees a byte too many.  Built by
// tests/test_decoder_cpu.py with g++ -fsanitize=address,undefined.
//
// stdin:  u64 n_steps, per step {u32 kind, flags, cp; u64 start, stop, a_len, b_len; a; b},
//         u64 n_docs, doc_tok[n_docs + 1], tok_off[n_tok + 1], the bytes
// stdout: u64 n_bytes, text_off[n_docs + 1], the text
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../csrc/decoder_internal.h"

using decoder::HostOp;
using decoder::In;
using decoder::Step;

namespace {

constexpr uint64_t kThreads = 256;

std::vector<uint8_t> g_in;
size_t g_at = 0;

void need(size_t n) {
  if (g_at + n > g_in.size()) {
    fprintf(stderr, "decoder_check: short input\n");
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
  Exact(Exact&& o) : p(o.p), n(o.n) { o.p = nullptr; }
  Exact& operator=(Exact&& o) {
    free(p);
    p = o.p;
    n = o.n;
    o.p = nullptr;
    return *this;
  }
  ~Exact() { free(p); }
};

struct Batch {
  Exact<uint8_t> bytes{0};
  Exact<uint64_t> tok_off{0}, doc_tok{0}, doc_off{0};
  uint64_t n = 0, n_tok = 0;
};

// one op over the batch, as decoder_host.cpp's run_op and the kernels of decoder.hip do it
Batch run_op(const HostOp& h, const Batch& cur, uint64_t n_docs) {
  Exact<uint8_t> sa(h.a.size()), sb(h.b.size());
  if (sa.n) memcpy(sa.p, h.a.data(), sa.n);
  if (sb.n) memcpy(sb.p, h.b.data(), sb.n);
  const Step st{h.op, h.flags, sa.p, sa.n, sb.p, sb.n};
  In in{};
  in.bytes = cur.bytes.p;
  in.n = cur.n;
  in.tok_off = cur.tok_off.p;
  in.n_tok = cur.n_tok;
  in.doc_tok = cur.doc_tok.p;
  in.n_docs = n_docs;
  in.doc_off = cur.doc_off.p;
  Exact<uint64_t> lo(n_docs), hi(n_docs), first(n_docs);
  Exact<uint8_t> cand(cur.n), mark(cur.n);
  if (mark.n) memset(mark.p, 0, mark.n);
  in.lo = lo.p;
  in.hi = hi.p;
  in.first = first.p;
  in.mark = mark.p;
  switch (h.prep) {
    case decoder::P_STRIP:
    case decoder::P_TRIM:
      for (uint64_t d = 0; d < n_docs; d++) {
        const uint64_t ds = in.doc_off[d], de = in.doc_off[d + 1];
        if (h.prep == decoder::P_STRIP) decoder::strip_range(in.bytes, st.a, st.a_len, h.start, h.stop, ds, de, &lo.p[d], &hi.p[d]);
        else decoder::trim_range(in.bytes, ds, de, &lo.p[d], &hi.p[d]);
      }
      break;
    case decoder::P_WP_FIRST:
      for (uint64_t d = 0; d < n_docs; d++) first.p[d] = decoder::wp_first(st, in, d);
      break;
    case decoder::P_REPLACE:
      for (uint64_t p = 0; p < in.n; p++) {
        const uint64_t d = decoder::doc_of(in.doc_off, n_docs, p);
        cand.p[p] = decoder::rep_cand(st, in.bytes, in.doc_off[d + 1], p);
      }
      for (uint64_t p = 0; p < in.n; p++) {
        if (!cand.p[p]) continue;
        const uint64_t d = decoder::doc_of(in.doc_off, n_docs, p);
        decoder::rep_chain(st, cand.p, mark.p, in.doc_off[d], in.doc_off[d + 1], p);
      }
      break;
    case decoder::P_CLEANUP:
      for (uint64_t p = 0; p < in.n; p++) {
        if (!decoder::is_set_byte(in.bytes[p])) continue;
        const uint64_t d = decoder::doc_of(in.doc_off, n_docs, p);
        decoder::cleanup_run(in.bytes, mark.p, in.doc_off[d], in.doc_off[d + 1], p);
      }
      break;
    default:
      break;
  }
  const uint64_t nu = decoder::n_units(st, in), nblk = (nu + 1 + kThreads - 1) / kThreads;
  const uint64_t* uoff = decoder::unit_off(st, in);
  // the count, per workgroup, and its scan
  std::vector<uint64_t> blk(nblk + 1, 0);
  for (uint64_t b = 0; b < nblk; b++)
    for (uint64_t u = b * kThreads; u < (b + 1) * kThreads && u < nu; u++)
      blk[b] += decoder::unit_emit(st, in, decoder::doc_of(uoff, n_docs, u), u, nullptr);
  uint64_t run = 0;
  for (uint64_t b = 0; b <= nblk; b++) {
    const uint64_t c = b < nblk ? blk[b] : 0;
    blk[b] = run;
    run += c;
  }
  const uint64_t tail = decoder::tail_len(st), total = blk[nblk] + n_docs * tail;
  // the write
  Batch out;
  out.bytes = Exact<uint8_t>(total);
  out.tok_off = Exact<uint64_t>(n_docs + 1);
  out.doc_off = Exact<uint64_t>(n_docs + 1);
  out.doc_tok = Exact<uint64_t>(n_docs + 1);
  out.n = total;
  out.n_tok = n_docs;
  std::vector<uint8_t> written(n_docs + 1, 0);
  for (uint64_t b = 0; b < nblk; b++) {
    const uint64_t bs = b * kThreads;
    uint64_t pre[kThreads], ex = 0;
    for (uint64_t t = 0; t < kThreads; t++) {
      const uint64_t u = bs + t;
      pre[t] = ex;
      if (u >= nu) continue;
      const uint64_t d = decoder::doc_of(uoff, n_docs, u);
      const uint64_t cnt = decoder::unit_emit(st, in, d, u, nullptr);
      if (cnt) {
        uint8_t* at = out.bytes.p + blk[b] + ex + d * tail;
        if (decoder::unit_emit(st, in, d, u, at) != cnt) exit(3);
      }
      ex += cnt;
    }
    for (uint64_t dd = decoder::first_doc_from(uoff, n_docs, bs); dd <= n_docs; dd++) {
      const uint64_t o = uoff[dd];
      if (o >= bs + kThreads) break;
      out.tok_off.p[dd] = blk[b] + pre[o - bs] + dd * tail;
      written[dd]++;
    }
  }
  for (uint64_t d = 0; d <= n_docs; d++)
    if (written[d] != 1) {
      fprintf(stderr, "decoder_check: offset %llu written %d times\n", (unsigned long long)d, (int)written[d]);
      exit(3);
    }
  if (tail)
    for (uint64_t d = 0; d < n_docs; d++) decoder::put(out.bytes.p + out.tok_off.p[d + 1] - tail, st.b, tail);
  if (out.tok_off.p[n_docs] != total) exit(3);
  for (uint64_t d = 0; d <= n_docs; d++) {
    out.doc_off.p[d] = out.tok_off.p[d];
    out.doc_tok.p[d] = d;
  }
  return out;
}

}  // namespace

int main() {
  {
    uint8_t tmp[1 << 16];
    size_t k;
    while ((k = fread(tmp, 1, sizeof tmp, stdin)) > 0) g_in.insert(g_in.end(), tmp, tmp + k);
  }
  std::vector<HostOp> ops;
  const uint64_t n_steps = rd64();
  for (uint64_t i = 0; i < n_steps; i++) {
    const uint32_t kind = rd32(), flags = rd32(), cp = rd32();
    const uint64_t start = rd64(), stop = rd64(), a_len = rd64(), b_len = rd64();
    const std::string a = rds(a_len), b = rds(b_len);
    const char* err = decoder::expand(kind, flags, a, b, cp, start, stop, &ops);
    if (err) {
      fprintf(stderr, "decoder_check: step %llu: %s\n", (unsigned long long)i, err);
      return 2;
    }
  }
  if (ops.empty()) decoder::expand(decoder::K_FUSE, 0, "", "", 0, 0, 0, &ops);
  const uint64_t n_docs = rd64();
  Batch cur;
  cur.doc_tok = Exact<uint64_t>(n_docs + 1);
  for (uint64_t d = 0; d <= n_docs; d++) cur.doc_tok.p[d] = rd64();
  cur.n_tok = cur.doc_tok.p[n_docs];
  cur.tok_off = Exact<uint64_t>(cur.n_tok + 1);
  for (uint64_t j = 0; j <= cur.n_tok; j++) cur.tok_off.p[j] = rd64();
  cur.n = cur.tok_off.p[cur.n_tok];
  cur.bytes = Exact<uint8_t>(cur.n);
  need(cur.n);
  if (cur.n) memcpy(cur.bytes.p, g_in.data() + g_at, cur.n);
  cur.doc_off = Exact<uint64_t>(n_docs + 1);
  for (uint64_t d = 0; d <= n_docs; d++) cur.doc_off.p[d] = cur.tok_off.p[cur.doc_tok.p[d]];
  for (const HostOp& h : ops) cur = run_op(h, cur, n_docs);
  fwrite(&cur.n, 8, 1, stdout);
  fwrite(cur.doc_off.p, 8, n_docs + 1, stdout);
  if (cur.n) fwrite(cur.bytes.p, 1, cur.n, stdout);
  return 0;
}
