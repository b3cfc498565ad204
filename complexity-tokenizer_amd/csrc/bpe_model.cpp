// tokenizer.json's `model` object as the reference reads it: model.vocab, model.merges through
// deserialize_merges and BpeTokenizer::new, handed to the table compiler as a BpeModel
// (table_compile.h).  Host-only and HIP-free, with the few helpers the loader and the compiler share.
//
// Reference counterparts (Complexity-ML/complexity-tokenizer v0.3.3):
//   loader            src/huggingface/mod.rs:32-116 (schema), :247-334
//   merge table       src/bpe.rs:52-79 (BpeTokenizer::new)
#include <sched.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <thread>

#include "json.hpp"
#include "table_compile.h"

namespace ctok_rt __attribute__((visibility("hidden"))) {

// CPUs this process may run on: the affinity mask capped by the cgroup v2 quota (cpu.max), as
// Rust's available_parallelism (rayon's default pool, reference src/huggingface/mod.rs:695)
// counts them on Linux.  Cached: read once per process.
unsigned usable_cpus_once() {
  static const unsigned n = [] {
    unsigned c = std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) c = std::max(1, CPU_COUNT(&set));
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
      char q[32] = {0};
      unsigned long long period = 0;
      if (fscanf(f, "%31s %llu", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
        const unsigned long long quota = strtoull(q, nullptr, 10);
        c = std::min<unsigned>(c, (unsigned)std::max<unsigned long long>(1, quota / period));
      }
      fclose(f);
    }
    return c;
  }();
  return n;
}

void LoadTimer::lap(const char* what) {
  if (!on) return;
  const auto now = std::chrono::steady_clock::now();
  fprintf(stderr, "[ctok load] %-12s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t0).count());
  t0 = now;
}

// ----------------------------------------------------------------------------- byte map
// GPT-2 bytes_to_unicode (src/pretokenizers.rs:130-153): byte -> code point
std::vector<uint32_t> byte_map() {
  std::vector<int> bs;
  for (int b = '!'; b <= '~'; b++) bs.push_back(b);
  for (int b = 0xA1; b <= 0xAC; b++) bs.push_back(b);
  for (int b = 0xAE; b <= 0xFF; b++) bs.push_back(b);
  std::vector<uint32_t> cs(bs.begin(), bs.end());
  uint32_t n = 0;
  std::vector<bool> in(256, false);
  for (int b : bs) in[b] = true;
  for (int b = 0; b < 256; b++)
    if (!in[b]) { bs.push_back(b); cs.push_back(256 + n++); }
  std::vector<uint32_t> m(256);
  for (size_t i = 0; i < 256; i++) m[bs[i]] = cs[i];
  return m;
}

std::vector<int> byte_unmap() {
  std::vector<int> inv(0x144, -1);
  const std::vector<uint32_t> bm = byte_map();
  for (int b = 0; b < 256; b++) inv[bm[b]] = b;
  return inv;
}

bool unmap_bytes(const std::vector<int>& inv, const std::vector<uint32_t>& cps, std::string& raw) {
  raw.clear();
  for (uint32_t c : cps) {
    if (c >= inv.size() || inv[c] < 0) return false;
    raw += (char)inv[c];
  }
  return true;
}

std::string utf8(uint32_t cp) {
  std::string o;
  if (cp < 0x80) o += (char)cp;
  else if (cp < 0x800) { o += (char)(0xC0 | (cp >> 6)); o += (char)(0x80 | (cp & 0x3F)); }
  else if (cp < 0x10000) { o += (char)(0xE0 | (cp >> 12)); o += (char)(0x80 | ((cp >> 6) & 0x3F)); o += (char)(0x80 | (cp & 0x3F)); }
  else { o += (char)(0xF0 | (cp >> 18)); o += (char)(0x80 | ((cp >> 12) & 0x3F)); o += (char)(0x80 | ((cp >> 6) & 0x3F)); o += (char)(0x80 | (cp & 0x3F)); }
  return o;
}

bool decode_utf8(const std::string& s, std::vector<uint32_t>& out) {
  out.clear();
  for (size_t i = 0; i < s.size();) {
    uint8_t b = (uint8_t)s[i];
    int len = b < 0x80 ? 1 : (b >> 5) == 6 ? 2 : (b >> 4) == 14 ? 3 : (b >> 3) == 30 ? 4 : 0;
    if (!len || i + len > s.size()) return false;
    uint32_t cp = len == 1 ? b : len == 2 ? (b & 0x1Fu) : len == 3 ? (b & 0x0Fu) : (b & 0x07u);
    for (int k = 1; k < len; k++) cp = (cp << 6) | ((uint8_t)s[i + k] & 0x3Fu);
    out.push_back(cp);
    i += len;
  }
  return true;
}

// ----------------------------------------------------------------------------- model
BpeModel parse_model(const ctj::Value& model, std::unordered_map<std::string, uint32_t>& vocab,
                     std::unordered_map<uint32_t, std::string>& id_to_token, LoadTimer& timer) {
  BpeModel m;
  m.vocab = &vocab;
  m.id_to_token = &id_to_token;
  const ctj::Value* vv = model.get("vocab");
  if (!vv) throw_err(CTOK_E_PARSE, "missing field `vocab`");
  if (vv->kind != ctj::Value::Object) throw_err(CTOK_E_PARSE, "invalid type for `vocab`, expected a map");
  vocab.reserve(vv->obj.size() * 2);
  std::vector<const std::string*> first_keys;  // first occurrence of each key, in file order
  first_keys.reserve(vv->obj.size());
  for (const auto& e : vv->obj) {
    if (!e.second.is_u32()) throw_err(CTOK_E_PARSE, "invalid value for vocab entry `" + e.first + "`, expected u32");
    auto ins = vocab.try_emplace(e.first, (uint32_t)e.second.u);
    if (ins.second) first_keys.push_back(&e.first);
    else ins.first->second = (uint32_t)e.second.u;  // HashMap insert: a later duplicate key wins
  }
  // Vocab::id_to_token (src/vocab.rs:47-52).  Several tokens sharing one id make the reference's
  // choice depend on HashMap order; here the later entry of the file wins (first occurrence of a
  // key, final value) -- parity for such files is unpinned.
  id_to_token.reserve(first_keys.size() * 2);
  for (const std::string* k : first_keys) {
    const uint32_t id = vocab.find(*k)->second;
    id_to_token[id] = *k;
    m.max_id = std::max(m.max_id, id);
  }
  timer.lap("vocab");
  // merges: deserialize_merges (mod.rs:56-101) then split(' ') == 2 parts (mod.rs:252-264)
  std::vector<std::pair<std::string, std::string>> merges;
  if (const ctj::Value* mv = model.get("merges")) {
    if (mv->kind != ctj::Value::Array) throw_err(CTOK_E_PARSE, "invalid type for `merges`, expected a sequence of strings or arrays of two strings");
    merges.reserve(mv->arr.size());
    for (const auto& it : mv->arr) {
      std::string s;
      if (it.kind == ctj::Value::String) s = it.s;
      else if (it.kind == ctj::Value::Array && it.arr.size() == 2 && it.arr[0].kind == ctj::Value::String &&
               it.arr[1].kind == ctj::Value::String) s = it.arr[0].s + " " + it.arr[1].s;
      else continue;
      size_t sp = s.find(' ');
      if (sp == std::string::npos || s.find(' ', sp + 1) != std::string::npos) continue;
      merges.emplace_back(s.substr(0, sp), s.substr(sp + 1));
    }
  }
  m.n_listed = merges.size();
  // BpeTokenizer::new (src/bpe.rs:52-79)
  std::unordered_map<uint64_t, uint32_t> ranks;  // (a<<32|b) -> rank, last duplicate wins
  ranks.reserve(merges.size() * 2);
  for (size_t r = 0; r < merges.size(); r++) {
    auto ia = vocab.find(merges[r].first);
    auto ib = vocab.find(merges[r].second);
    if (ia == vocab.end() || ib == vocab.end()) continue;
    auto in = vocab.find(merges[r].first + merges[r].second);
    if (in == vocab.end()) continue;
    ranks[((uint64_t)ia->second << 32) | ib->second] = (uint32_t)r;
    m.valid_new.push_back(in->second);
  }
  m.merges.reserve(ranks.size());
  for (const auto& kv : ranks) m.merges.push_back({kv.second, (uint32_t)(kv.first >> 32), (uint32_t)kv.first});
  std::sort(m.merges.begin(), m.merges.end(), [](const BpeModel::Merge& x, const BpeModel::Merge& y) { return x.rank < y.rank; });
  // byte-level initial ids: vocab[bytes_to_unicode[b]] (src/bpe.rs:94-97), -1 = dropped
  const std::vector<uint32_t> bm = byte_map();
  for (int b = 0; b < 256; b++) {
    auto it = vocab.find(utf8(bm[b]));
    m.byte2id[b] = it == vocab.end() ? -1 : (int32_t)it->second;
  }
  timer.lap("ranks");
  return m;
}

}  // namespace ctok_rt
