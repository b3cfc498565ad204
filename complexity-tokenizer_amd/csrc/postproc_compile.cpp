// The template compiler of the PostProcessor: see postproc_internal.h.  Host-only.
#include "postproc_internal.h"

namespace postproc {

namespace {

struct Char {
  uint32_t cp;
  size_t at;  // its first byte
};

// the chars of well-formed UTF-8 (is_utf8 has said so)
std::vector<Char> chars_of(const std::string& s) {
  std::vector<Char> out;
  const uint8_t* t = (const uint8_t*)s.data();
  for (size_t i = 0; i < s.size();) {
    const uint8_t b = t[i];
    const uint32_t len = b < 0x80 ? 1 : b < 0xE0 ? 2 : b < 0xF0 ? 3 : 4;
    uint32_t cp = len == 1 ? b : b & (0xFFu >> (len + 1));
    for (uint32_t j = 1; j < len; j++) cp = (cp << 6) | (t[i + j] & 0x3F);
    out.push_back(Char{cp, i});
    i += len;
  }
  return out;
}

// char::is_whitespace: the White_Space property
bool is_space(uint32_t c) {
  return (c >= 0x09 && c <= 0x0D) || c == 0x20 || c == 0x85 || c == 0xA0 || c == 0x1680 || (c >= 0x2000 && c <= 0x200A) ||
         c == 0x2028 || c == 0x2029 || c == 0x202F || c == 0x205F || c == 0x3000;
}

// template_process, postprocessors.rs:88-148
void walk(const std::string& tmpl, const HostStep& st, bool has_pair, std::vector<HostItem>* out) {
  const std::vector<Char> ch = chars_of(tmpl);
  const size_t n = ch.size();
  auto byte_at = [&](size_t i) { return i < n ? ch[i].at : tmpl.size(); };
  size_t i = 0;
  while (i < n) {
    if (ch[i].cp == '$' && i + 1 < n) {
      if (ch[i + 1].cp == 'A') {
        out->push_back(HostItem{IT_A, 0});
        i += 2;
      } else if (ch[i + 1].cp == 'B') {
        if (has_pair) out->push_back(HostItem{IT_B, 0});
        i += 2;
      } else {
        i += 1;
      }
    } else if (ch[i].cp == '<' || ch[i].cp == '[') {
      const uint32_t end = ch[i].cp == '<' ? '>' : ']';
      size_t lo = i;
      while (i < n && ch[i].cp != end) i++;
      if (i < n) i++;
      size_t hi = i;  // str::trim of chars[lo .. hi)
      while (lo < hi && is_space(ch[lo].cp)) lo++;
      while (hi > lo && is_space(ch[hi - 1].cp)) hi--;
      const std::string token = tmpl.substr(byte_at(lo), byte_at(hi) - byte_at(lo));
      for (const auto& sp : st.specials)
        if (sp.first == token) {
          out->push_back(HostItem{IT_SPECIAL, sp.second});
          break;
        }
    } else {
      i += 1;
    }
  }
}

void finish(HostList* l) {
  const size_t n = l->items.size();
  l->pa.assign(n + 1, 0);
  l->pb.assign(n + 1, 0);
  l->ps.assign(n + 1, 0);
  l->val.assign(n, 0);
  for (size_t k = 0; k < n; k++) {
    const HostItem& it = l->items[k];
    l->pa[k + 1] = l->pa[k] + (it.kind == IT_A);
    l->pb[k + 1] = l->pb[k] + (it.kind == IT_B);
    l->ps[k + 1] = l->ps[k] + (it.kind == IT_SPECIAL);
    l->val[k] = it.kind == IT_SPECIAL ? it.value : 0;
  }
}

CompileError too_many(uint64_t n, size_t step, std::string* err) {
  *err = "postprocessor: step " + std::to_string(step) + " makes a flat list of " + std::to_string(n) + " items, the limit is " +
         std::to_string(kMaxItems);
  return C_CAPACITY;
}

CompileError compile_list(const std::vector<HostStep>& steps, bool has_pair, HostList* out, std::string* err) {
  std::vector<HostItem> cur;
  if (steps.empty()) cur.push_back(HostItem{IT_A, 0});  // the ids; the pair is dropped
  for (size_t k = 0; k < steps.size(); k++) {
    // (Sequence: pair_result.take() -- the pair goes to the first step only)
    const std::vector<HostItem> t = step_items(steps[k], k == 0 && has_pair);
    if (k == 0) {
      if (t.size() > kMaxItems) return too_many(t.size(), k, err);
      cur = t;
      continue;
    }
    uint64_t n_a = 0;
    for (const HostItem& it : t) n_a += it.kind == IT_A;
    const uint64_t n_new = n_a * cur.size() + (t.size() - n_a);  // (at most 4096 * the template's chars)
    if (n_new > kMaxItems) return too_many(n_new, k, err);
    std::vector<HostItem> next;
    next.reserve(n_new);
    for (const HostItem& it : t) {
      if (it.kind == IT_A) next.insert(next.end(), cur.begin(), cur.end());
      else if (it.kind == IT_SPECIAL) next.push_back(it);
    }
    cur.swap(next);
  }
  out->items = cur;
  finish(out);
  return C_OK;
}

}  // namespace

bool is_utf8(const std::string& s) {
  const uint8_t* t = (const uint8_t*)s.data();
  const size_t n = s.size();
  for (size_t i = 0; i < n;) {
    const uint8_t b = t[i];
    if (b < 0x80) {
      i++;
      continue;
    }
    uint32_t len, cp;
    if (b >= 0xC2 && b < 0xE0) len = 2, cp = b & 0x1F;
    else if (b >= 0xE0 && b < 0xF0) len = 3, cp = b & 0x0F;
    else if (b >= 0xF0 && b < 0xF5) len = 4, cp = b & 0x07;
    else return false;
    if (i + len > n) return false;
    for (uint32_t j = 1; j < len; j++) {
      if ((t[i + j] & 0xC0) != 0x80) return false;
      cp = (cp << 6) | (t[i + j] & 0x3F);
    }
    if (len == 3 && (cp < 0x800 || (cp >= 0xD800 && cp < 0xE000))) return false;
    if (len == 4 && (cp < 0x10000 || cp > 0x10FFFF)) return false;
    i += len;
  }
  return true;
}

std::vector<HostItem> step_items(const HostStep& st, bool has_pair) {
  std::vector<HostItem> out;
  switch (st.kind) {
    case K_TEMPLATE:
      walk(has_pair && st.has_pair_template ? st.pair : st.single, st, has_pair, &out);
      break;
    case K_BERT:  // cls ids sep [pair sep]
      out = {HostItem{IT_SPECIAL, st.id_a}, HostItem{IT_A, 0}, HostItem{IT_SPECIAL, st.id_b}};
      if (has_pair) {
        out.push_back(HostItem{IT_B, 0});
        out.push_back(HostItem{IT_SPECIAL, st.id_b});
      }
      break;
    case K_ROBERTA:  // bos ids eos [eos pair eos]
      out = {HostItem{IT_SPECIAL, st.id_a}, HostItem{IT_A, 0}, HostItem{IT_SPECIAL, st.id_b}};
      if (has_pair) {
        out.push_back(HostItem{IT_SPECIAL, st.id_b});
        out.push_back(HostItem{IT_B, 0});
        out.push_back(HostItem{IT_SPECIAL, st.id_b});
      }
      break;
    default:
      break;
  }
  return out;
}

CompileError compile(const std::vector<HostStep>& steps, Program* out, std::string* err) {
  for (size_t k = 0; k < steps.size(); k++) {
    const HostStep& st = steps[k];
    if (st.kind >= K_N) {
      *err = "postprocessor step " + std::to_string(k) + ": no such post-processor";
      return C_ARG;
    }
    bool ok = is_utf8(st.single) && is_utf8(st.pair);
    for (const auto& sp : st.specials) ok = ok && is_utf8(sp.first);
    if (!ok) {
      *err = "postprocessor step " + std::to_string(k) + ": a string is not valid UTF-8";
      return C_ARG;
    }
  }
  CompileError e = compile_list(steps, false, &out->single, err);
  if (e != C_OK) return e;
  return compile_list(steps, true, &out->pair, err);
}

}  // namespace postproc
