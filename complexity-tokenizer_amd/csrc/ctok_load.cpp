// The tokenizer.json loader of the host runtime -- everything around the model: added tokens,
// normalizer, pre-tokenizer, post-processor, decoder -- and the C ABI functions that read only the
// loaded tokenizer (struct ctok).  The model itself is read by bpe_model.cpp and compiled into the
// device tables by table_compile.cpp.  Host-only: no HIP runtime call.
//
// Reference counterparts (Complexity-ML/complexity-tokenizer v0.3.3):
//   loader            src/huggingface/mod.rs:32-116 (schema), :159-166 (from_file), :247-334
//   normaliser choice src/huggingface/parsing.rs:10-90 (NFC default at :89)
//   pre-tokenizer     src/huggingface/parsing.rs:92-190; src/pretokenizers.rs:71-126, :298-302
//   vocab getters     src/vocab.rs:34-100, src/huggingface/mod.rs:856-866
//   decode table      src/huggingface/mod.rs:698-785, src/decoders.rs:74-119, parsing.rs:272-364
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string_view>
#include <unordered_set>

#include "gen/regex_props.h"
#include "gen/unicode_data.h"
#include "host_internal.h"
#include "knobs.h"
#include "rust_regex.h"

namespace ctok_rt __attribute__((visibility("hidden"))) {

int host_cls(uint32_t cp) {
  if (cp >= 0x110000) return 3;
  uint32_t w = ct_cls_stage2[ct_cls_stage1[cp >> 8] * 64 + ((cp & 255) >> 2)];
  return (w >> ((cp & 3) * 2)) & 3;
}

// Can the raw byte string `pat` occur inside one GPT2_PATTERN piece?  Pieces are: a run of
// White_Space; an optional leading U+0020 plus a run of one class among {L, N, other}; or a
// contraction 's 't 're 've 'm 'll 'd.  Conservative: true unless provably impossible.
bool can_occur_in_piece(const std::string& pat) {
  if (pat.empty()) return true;
  static const char* con[] = {"'s", "'t", "'re", "'ve", "'m", "'ll", "'d"};
  for (const char* c : con)
    if (std::string(c).find(pat) != std::string::npos) return true;
  size_t i = 0;
  bool lead_partial = false;
  while (i < pat.size() && ((uint8_t)pat[i] & 0xC0) == 0x80) { i++; lead_partial = true; }
  std::vector<int> cls;
  std::vector<uint32_t> cps;
  while (i < pat.size()) {
    uint8_t b = (uint8_t)pat[i];
    int len = b < 0x80 ? 1 : (b >> 5) == 6 ? 2 : (b >> 4) == 14 ? 3 : 4;
    if (i + len > pat.size()) break;  // trailing partial code point: class unknown
    uint32_t cp = len == 1 ? b : len == 2 ? (b & 0x1Fu) : len == 3 ? (b & 0x0Fu) : (b & 0x07u);
    for (int k = 1; k < len; k++) cp = (cp << 6) | ((uint8_t)pat[i + k] & 0x3Fu);
    cps.push_back(cp);
    cls.push_back(host_cls(cp));
    i += len;
  }
  if (cls.empty()) return true;
  bool all_ws = std::all_of(cls.begin(), cls.end(), [](int c) { return c == 0; });
  if (all_ws) return true;
  size_t k = 0;
  if (!lead_partial && cps[0] == ' ') k = 1;
  int want = -1;
  for (; k < cls.size(); k++) {
    if (cls[k] == 0) return false;
    if (want < 0) want = cls[k];
    else if (cls[k] != want) return false;
  }
  return true;
}

bool get_bool_field(const ctj::Value& o, const char* k, bool dflt, const char* ctx) {
  const ctj::Value* v = o.get(k);
  if (!v) return dflt;
  if (v->kind != ctj::Value::Bool) throw_err(CTOK_E_PARSE, std::string("invalid type for `") + k + "` in " + ctx + ", expected a boolean");
  return v->b;
}

// parse_normalizer (src/huggingface/parsing.rs:10-90): 1 = NFC, 0 = none
int parse_normalizer(const ctj::Value* v) {
  if (v && v->kind == ctj::Value::Object) {
    const ctj::Value* t = v->get("type");
    if (t) {
      std::string ty = t->kind == ctj::Value::String ? t->s : "";
      if (ty == "NFC") return 1;
      if (ty == "Sequence") {
        const ctj::Value* ns = v->get("normalizers");
        if (!ns || ns->kind != ctj::Value::Array) return 0;
        int any = 0;
        for (const auto& n : ns->arr) any |= parse_normalizer(&n);  // NFC is idempotent
        return any;
      }
      static const char* unsup[] = {"NFD", "NFKC", "NFKD", "Lowercase", "Strip", "StripAccents", "Replace",
                                    "Prepend", "BertNormalizer", "Precompiled"};
      for (const char* u : unsup)
        if (ty == u) throw_err(CTOK_E_UNSUPPORTED, "normalizer `" + ty + "` is outside the encode hot path (only NFC / none)");
      return 0;
    }
  }
  return 1;  // null, absent, or an object without "type": NFC (parsing.rs:89)
}

bool is_white_space(uint32_t c) {  // Unicode White_Space (Rust char::is_whitespace)
  return (c >= 9 && c <= 13) || c == 32 || c == 0x85 || c == 0xA0 || c == 0x1680 || (c >= 0x2000 && c <= 0x200A) ||
         c == 0x2028 || c == 0x2029 || c == 0x202F || c == 0x205F || c == 0x3000;
}

std::string encode_utf8(const std::vector<uint32_t>& cps, size_t a, size_t b) {
  std::string s;
  for (size_t i = a; i < b; i++) s += utf8(cps[i]);
  return s;
}

// parse_post_processor (src/huggingface/parsing.rs:193-253) and PostProcessor::process(ids, None)
// (src/postprocessors.rs:34-147), compiled to a list of items: kPadItemA = the sequence's ids,
// anything else = one special id.  The encode paths only ever call process(ids, None), so a
// template's $B and the pair template are never used.  "Sequence" and other types -> None.
void parse_post_processor(ctok* t, const ctj::Value* v) {
  t->has_pp = false;
  t->pp_items.clear();
  t->pp_kind = 0;
  if (!v || v->kind != ctj::Value::Object) return;
  const ctj::Value* ty = v->get("type");
  if (!ty) return;
  const std::string kind = ty->kind == ctj::Value::String ? ty->s : "";
  auto special = [&](const std::string& name, bool* found) -> uint32_t {
    for (const auto& e : t->special)
      if (e.first == name) {
        *found = true;
        return e.second;
      }
    *found = false;
    return 0;
  };
  if (kind == "TemplateProcessing") {
    std::string tpl = "<s> $A </s>";
    const ctj::Value* single = v->get("single");
    if (single && single->kind == ctj::Value::Array) {  // template_from_array (parsing.rs:236-253)
      std::vector<std::string> parts;
      for (const auto& item : single->arr) {
        if (item.kind != ctj::Value::Object) continue;
        if (const ctj::Value* sp = item.get("SpecialToken")) {
          const ctj::Value* id = sp->get("id");
          if (id && id->kind == ctj::Value::String) parts.push_back(id->s);
          continue;
        }
        if (const ctj::Value* sq = item.get("Sequence")) {
          const ctj::Value* id = sq->get("id");
          if (id && id->kind == ctj::Value::String) parts.push_back("$" + id->s);
        }
      }
      tpl.clear();
      for (size_t i = 0; i < parts.size(); i++) tpl += (i ? " " : "") + parts[i];
    }
    t->pp_single = tpl;
    if (const ctj::Value* pair = v->get("pair")) {
      if (pair->kind == ctj::Value::Array) {
        std::string ps;
        bool first = true;
        for (const auto& item : pair->arr) {
          if (item.kind != ctj::Value::Object) continue;
          std::string part;
          bool ok = false;
          if (const ctj::Value* sp = item.get("SpecialToken")) {
            const ctj::Value* id = sp->get("id");
            if (id && id->kind == ctj::Value::String) part = id->s, ok = true;
          } else if (const ctj::Value* sq = item.get("Sequence")) {
            const ctj::Value* id = sq->get("id");
            if (id && id->kind == ctj::Value::String) part = "$" + id->s, ok = true;
          }
          if (ok) {
            ps += (first ? "" : " ") + part;
            first = false;
          }
        }
        t->pp_pair = ps;
        t->pp_has_pair = true;
      }
    }
    t->pp_kind = 1;
    std::vector<uint32_t> ch;
    if (!decode_utf8(tpl, ch)) throw_err(CTOK_E_PARSE, "post_processor template is not valid UTF-8");
    size_t i = 0;  // template_process's walk (postprocessors.rs:103-144)
    while (i < ch.size()) {
      if (ch[i] == '$' && i + 1 < ch.size()) {
        if (ch[i + 1] == 'A') t->pp_items.push_back(kPadItemA);
        if (ch[i + 1] == 'A' || ch[i + 1] == 'B') i += 2;  // $B: the pair, absent in process(ids, None)
        else i += 1;
      } else if (ch[i] == '<' || ch[i] == '[') {
        const uint32_t end = ch[i] == '<' ? '>' : ']';
        const size_t a = i;
        while (i < ch.size() && ch[i] != end) i++;
        if (i < ch.size()) i++;  // include the end char
        size_t b = i;
        while (b > a && is_white_space(ch[b - 1])) b--;  // str::trim (the start is '<' or '[')
        bool found;
        const uint32_t id = special(encode_utf8(ch, a, b), &found);
        if (found) t->pp_items.push_back(id);
      } else {
        i++;
      }
    }
    t->has_pp = true;
  } else if (kind == "RobertaProcessing" || kind == "BertProcessing") {  // parsing.rs:221-236
    const bool roberta = kind == "RobertaProcessing";
    bool f;
    uint32_t a = special(roberta ? "<s>" : "[CLS]", &f);
    if (!f) a = roberta ? 0 : 101;
    uint32_t b = special(roberta ? "</s>" : "[SEP]", &f);
    if (!f) b = roberta ? 2 : 102;
    t->pp_items = {a, kPadItemA, b};  // roberta_process / bert_process with no pair
    t->has_pp = true;
    t->pp_kind = roberta ? 2 : 3;
  }
}

// Does the Rust regex crate compile pattern p?  The reference compiles a Split's pattern and, when
// Regex::new fails, leaves the text unsplit (src/pretokenizers.rs:277-302): the Split is a no-op.
// The crate (regex ^1.10, Cargo.toml:19; the regex-syntax grammar) has no look-around,
// backreferences, atomic groups, branch resets, comments or conditionals, rejects unknown escapes,
// a repetition with nothing to repeat, an inverted {n,m}, unbalanced groups / classes, unknown ASCII
// classes and \p{..} names that are not Unicode property names or values (UAX #44 loose matching;
// gen/regex_props.h, from the `regex` module's tables: a superset of the crate's).  This walks the
// pattern with that grammar and returns the first construct the crate rejects, "" when there is
// none.  It errs one way only: what it cannot decide counts as compiling (verbose-mode patterns,
// hex escapes, Age=), and a compiling Split is refused by the loader (CTOK_E_UNSUPPORTED), never
// silently dropped.  Possessive quantifiers (a++) are a repetition of a repetition to regex-syntax:
// they compile.  Restated for the tests by oracle/rust_regex.py.
namespace rxs {

std::string canon(std::string_view s) {
  std::string o;
  for (char c : s)
    if (c != ' ' && c != '_' && c != '-' && c != '\t' && c != '\n') o += (char)toupper((unsigned char)c);
  return o;
}

template <size_t N>
bool in_table(const char* const (&tab)[N], const std::string& k) {
  return std::binary_search(tab, tab + N, k.c_str(), [](const char* a, const char* b) { return strcmp(a, b) < 0; });
}

bool single_known(const std::string& c) {
  if (in_table(ct_prop_single, c)) return true;
  return c.size() > 2 && c.compare(0, 2, "IS") == 0 && in_table(ct_prop_single, c.substr(2));  // "is" prefix
}

// \p{body}: a property the crate may know (name=value for gc / sc / scx / gcb / wb / sb, age
// taken as known; other properties the tables know: taken as known, a name they do not: unknown)
bool property_known(std::string_view body) {
  for (std::string_view sep : {std::string_view("!="), std::string_view("="), std::string_view(":")}) {
    const size_t at = body.find(sep);
    if (at == std::string_view::npos) continue;
    std::string k = canon(body.substr(0, at)), v = canon(body.substr(at + sep.size()));
    if (k == "AGE") return true;
    static const std::map<std::string, std::string> kv = {
        {"GC", "GC"}, {"GENERALCATEGORY", "GC"}, {"SC", "SC"}, {"SCRIPT", "SC"}, {"SCX", "SCX"},
        {"SCRIPTEXTENSIONS", "SCX"}, {"GCB", "GCB"}, {"GRAPHEMECLUSTERBREAK", "GCB"}, {"WB", "WB"},
        {"WORDBREAK", "WB"}, {"SB", "SB"}, {"SENTENCEBREAK", "SB"}};
    auto it = kv.find(k);
    if (it != kv.end()) return in_table(ct_prop_kv, it->second + "=" + v);
    return in_table(ct_prop_other, k);
  }
  return single_known(canon(body));
}

}  // namespace rxs

std::string rust_regex_rejects(const std::string& p) {
  const size_t n = p.size();
  size_t i = 0;
  int depth = 0;
  std::vector<bool> empty{true};  // per open group: nothing to repeat yet
  auto is_alnum = [](char c) { return isalnum((unsigned char)c) != 0; };
  // at p[j] == '\\' (inside or outside a class): "" or the reason; j moves past the escape
  auto escape = [&](size_t& j) -> std::string {
    if (j + 1 >= n) return "trailing backslash";
    const char c = p[j + 1];
    if (c >= '1' && c <= '9') return std::string("backreference \\") + c;
    if (c == 'k') return "named backreference \\k";
    if (c == 'g') return "backreference \\g";
    if (c == 'p' || c == 'P') {
      if (j + 2 >= n) return "incomplete \\p escape";
      if (p[j + 2] == '{') {
        const size_t e = p.find('}', j + 3);
        if (e == std::string::npos) return "unclosed \\p{";
        const std::string body = p.substr(j + 3, e - j - 3);
        j = e + 1;
        return rxs::property_known(body) ? "" : "unknown Unicode property \\p{" + body + "}";
      }
      const std::string body(1, p[j + 2]);
      j += 3;
      return rxs::property_known(body) ? "" : "unknown Unicode property \\p" + body;
    }
    j += 2;
    if (c == 'x' || c == 'u' || c == 'U') return "";  // (hex escapes: taken as valid)
    if (is_alnum(c) && !strchr("aftnrvAzbBdDsSwW", c)) return std::string("unrecognized escape \\") + c;
    return "";
  };
  while (i < n) {
    const char c = p[i];
    if (c == '\\') {
      const std::string why = escape(i);
      if (!why.empty()) return why;
      empty.back() = false;
      continue;
    }
    if (c == '[') {  // class: nested classes, escapes, [:name:]; a leading ']' is literal
      size_t j = i + 1;
      if (j < n && p[j] == '^') j++;
      if (j < n && p[j] == ']') j++;
      int cd = 1;
      while (j < n && cd) {
        const char d = p[j];
        if (d == '\\') {
          const std::string why = escape(j);
          if (!why.empty()) return why;
          continue;
        }
        if (d == '[' && j + 1 < n && p[j + 1] == ':') {
          // [:name:] with a known name is an ASCII class; with any other name regex-syntax
          // (maybe_parse_ascii_class) backtracks and reads the '[' as a nested class
          const size_t e = p.find(":]", j + 2);
          if (e != std::string::npos) {
            std::string nm = p.substr(j + 2, e - j - 2);
            if (!nm.empty() && nm[0] == '^') nm.erase(0, 1);
            static const char* const kAscii[] = {"alnum", "alpha", "ascii", "blank", "cntrl", "digit", "graph",
                                                 "lower", "print", "punct", "space", "upper", "word", "xdigit"};
            if (std::find_if(std::begin(kAscii), std::end(kAscii), [&](const char* a) { return nm == a; }) != std::end(kAscii)) {
              j = e + 2;
              continue;
            }
          }
        }
        if (d == '[') {
          cd++;
          j++;
          if (j < n && p[j] == '^') j++;
          if (j < n && p[j] == ']') j++;
          continue;
        }
        if (d == ']') cd--;
        j++;
      }
      if (cd) return "unclosed character class";
      i = j;
      empty.back() = false;
      continue;
    }
    if (c == '(') {
      if (i + 1 < n && p[i + 1] == '?') {
        const std::string_view rest = std::string_view(p).substr(i + 2);
        auto starts = [&](const char* s) { return rest.compare(0, strlen(s), s) == 0; };
        if (starts("=") || starts("!")) return std::string("look-ahead (?") + rest[0];
        if (starts("<=") || starts("<!")) return "look-behind (?" + std::string(rest.substr(0, 2));
        if (starts(">")) return "atomic group (?>";
        if (starts("P=")) return "named backreference (?P=";
        if (!rest.empty() && (strchr("|#('&+0", rest[0]) || isdigit((unsigned char)rest[0])))
          return std::string("unsupported group (?") + rest[0];
        if (starts("P<") || starts("<")) {
          const size_t k = i + 2 + (starts("P<") ? 2 : 1);
          const size_t e = p.find('>', k);
          if (e == std::string::npos) return "unclosed group name";
          const std::string name = p.substr(k, e - k);
          bool ok = !name.empty() && (isalpha((unsigned char)name[0]) || name[0] == '_');
          for (char ch : name) ok = ok && (is_alnum(ch) || ch == '_' || ch == '.' || ch == '[' || ch == ']');
          if (!ok) return "invalid group name " + name;
          i = e + 1;
        } else {  // flags: (?flags) or (?flags:...)
          size_t k = i + 2;
          while (k < n && strchr("imsxuUR-", p[k])) {
            if (p[k] == 'x') return "";  // verbose mode (comments, ignored space): not walked; taken as compiling
            k++;
          }
          if (k >= n || (p[k] != ':' && p[k] != ')')) return std::string("unrecognized flag ") + (k < n ? p.substr(k, 1) : "(end)");
          i = k + 1;
          if (p[k] == ')') continue;
        }
      } else {
        i++;
      }
      depth++;
      empty.push_back(true);
      continue;
    }
    if (c == ')') {
      if (--depth < 0) return "unbalanced ')'";
      empty.pop_back();
      empty.back() = false;
      i++;
      continue;
    }
    if (c == '|') {
      empty.back() = true;
      i++;
      continue;
    }
    if (c == '*' || c == '+' || c == '?') {
      if (empty.back()) return "repetition operator missing expression";
      i++;
      continue;
    }
    if (c == '{') {  // counted repetition {n}, {n,}, {n,m}; anything else is not walked further
      const size_t e = p.find('}', i);
      if (e != std::string::npos) {
        const std::string body = p.substr(i + 1, e - i - 1);
        const size_t comma = body.find(',');
        const std::string a = body.substr(0, comma), b = comma == std::string::npos ? "" : body.substr(comma + 1);
        auto digits = [](const std::string& s) { return !s.empty() && std::all_of(s.begin(), s.end(), ::isdigit); };
        // a count is a u32 (regex-syntax parse_decimal): a longer one is an invalid decimal
        auto count = [](const std::string& s) -> uint64_t {
          uint64_t v = 0;
          for (char ch : s) {
            v = v * 10 + (uint64_t)(ch - '0');
            if (v > 0xFFFFFFFFull) return ~(uint64_t)0;
          }
          return v;
        };
        if (digits(a) && (comma == std::string::npos || b.empty() || digits(b))) {
          if (empty.back()) return "repetition operator missing expression";
          if (count(a) == ~(uint64_t)0 || (!b.empty() && count(b) == ~(uint64_t)0)) return "repetition count overflows u32 {" + body + "}";
          if (!b.empty() && count(b) < count(a)) return "invalid repetition range {" + body + "}";
          i = e + 1;
          continue;
        }
      }
      empty.back() = false;
      i++;
      continue;
    }
    empty.back() = false;
    i++;
  }
  if (depth) return "unclosed group";
  return "";
}

// flattens parse_pre_tokenizer (src/huggingface/parsing.rs:92-190) into the supported chain:
// no-op Splits (patterns the Rust regex crate rejects, src/pretokenizers.rs:298-302) around
// exactly one ByteLevel.  kinds: 'B' ByteLevel, 'S' no-op split
void parse_pre_tokenizer(const ctj::Value* v, std::vector<std::pair<char, bool>>& chain, int depth) {
  if (!(v && v->kind == ctj::Value::Object && v->get("type"))) {
    if (depth == 0) { chain.push_back({'B', false}); return; }  // default ByteLevel(false)
    throw_err(CTOK_E_UNSUPPORTED, "pre_tokenizer entry without a type");
  }
  const ctj::Value* t = v->get("type");
  std::string ty = t->kind == ctj::Value::String ? t->s : "";
  if (ty == "ByteLevel") {
    const ctj::Value* a = v->get("add_prefix_space");
    chain.push_back({'B', a && a->kind == ctj::Value::Bool ? a->b : false});
  } else if (ty == "Split") {
    std::string pat;
    const ctj::Value* p = v->get("pattern");
    if (p && p->kind == ctj::Value::Object) {
      const ctj::Value* r = p->get("Regex");
      if (r && r->kind == ctj::Value::String) pat = r->s;
    }
    if (rust_regex_rejects(pat).empty())
      throw_err(CTOK_E_UNSUPPORTED, "Split pre-tokenizer with a pattern the Rust regex crate compiles is outside the "
                                    "encode hot path: nothing the crate rejects (look-around, backreference, atomic "
                                    "group, unknown escape or \\p{..} name, unbalanced group / class) was found, so "
                                    "the pattern is taken as compiling (pattern: " + pat + ")");
    chain.push_back({'S', false});
  } else if (ty == "Sequence" && depth == 0) {
    const ctj::Value* ps = v->get("pretokenizers");
    if (!ps || ps->kind != ctj::Value::Array || ps->arr.empty())
      throw_err(CTOK_E_UNSUPPORTED, "empty pre_tokenizer Sequence (no byte-level split)");
    for (const auto& e : ps->arr) parse_pre_tokenizer(&e, chain, depth + 1);
  } else {
    throw_err(CTOK_E_UNSUPPORTED, "pre_tokenizer `" + ty + "` is outside the encode hot path (ByteLevel only)");
  }
}


// parse_decoder (src/huggingface/parsing.rs:272-364) reduced to what decode needs: 1 = ByteLevel
// (also the default for a null / absent / non-object value or an object without "type"),
// 0 = None (an unknown type string: BpeTokenizer::decode joins the raw vocab strings,
// src/huggingface/mod.rs:737-740), -1 = a decoder outside the ByteLevel-BPE path.  In a
// Sequence, entries that parse to None are dropped (filter_map), Fuse is the identity on the
// one-string list the previous decoder leaves, and one ByteLevel is the whole effect.
int parse_decoder(const ctj::Value* v, std::string& name) {
  if (!v || v->kind != ctj::Value::Object) return 1;
  const ctj::Value* ty = v->get("type");
  if (!ty) return 1;
  const std::string t = ty->kind == ctj::Value::String ? ty->s : "";
  if (t == "ByteLevel") return 1;
  if (t == "Fuse") return 0;
  if (t == "Metaspace" || t == "WordPiece" || t == "BPE" || t == "CTC" || t == "Strip") { name = t; return -1; }
  if (t != "Sequence") return 0;
  const ctj::Value* decs = v->get("decoders");
  if (!decs || decs->kind != ctj::Value::Array || decs->arr.empty()) return 0;
  int nbl = 0, kept = 0;
  for (const auto& d : decs->arr) {
    std::string sub;
    const int k = parse_decoder(&d, sub);
    if (k < 0) { name = sub; return -1; }
    const ctj::Value* dt = d.kind == ctj::Value::Object ? d.get("type") : nullptr;
    const bool fuse = dt && dt->kind == ctj::Value::String && dt->s == "Fuse";
    if (k == 0 && !fuse) continue;  // None: dropped by filter_map
    kept++;
    if (k == 1) nbl++;
  }
  if (!kept) return 0;
  if (nbl > 1) { name = "Sequence with more than one ByteLevel"; return -1; }
  return nbl;
}

// Per-id decoded bytes: the ByteLevel decoder maps every char of the token back to a byte ('Ġ'
// and the 255 other GPT-2 chars, src/decoders.rs:74-92,101-107), keeps other ASCII chars
// (:108-110) and drops the rest; the raw decoder keeps the token's UTF-8 bytes.
void build_decode_table(ctok* t) {
  uint32_t n_ent = 0;
  for (const auto& kv : t->id_to_token) n_ent = std::max(n_ent, kv.first + 1);
  if (n_ent > (1u << 26)) throw_err(CTOK_E_UNSUPPORTED, "token ids above 2^26 are not supported by the decode table");
  const std::vector<int> inv = byte_unmap();  // GPT-2 char -> byte
  std::unordered_set<std::string> special;
  for (const auto& sp : t->special) special.insert(sp.first);
  t->dec_ent.assign(2 * (size_t)n_ent, 0);
  t->dec_bytes.clear();
  std::vector<uint32_t> cps;
  std::string out;
  for (uint32_t id = 0; id < n_ent; id++) {
    auto it = t->id_to_token.find(id);
    if (it == t->id_to_token.end()) continue;
    const std::string& tok = it->second;
    out.clear();
    if (t->decoder == 1) {
      if (!decode_utf8(tok, cps)) throw_err(CTOK_E_PARSE, "vocab entry is not valid UTF-8");
      for (uint32_t c : cps) {
        if (c < inv.size() && inv[c] >= 0) out += (char)inv[c];
        else if (c < 0x80) out += (char)c;
      }
    } else {
      out = tok;
    }
    if (out.size() > kDecLenMask) throw_err(CTOK_E_UNSUPPORTED, "vocab entry longer than 16 MiB");
    uint32_t y = (uint32_t)out.size();
    for (unsigned char c : out)
      if (c >= 0x80) { y |= kDecNonAscii; break; }
    if (special.count(tok)) y |= kDecSpecial;
    while (t->dec_bytes.size() & 3) t->dec_bytes.push_back(0);
    t->dec_ent[2 * id] = (uint32_t)t->dec_bytes.size();
    t->dec_ent[2 * id + 1] = y;
    t->dec_bytes.insert(t->dec_bytes.end(), out.begin(), out.end());
  }
  for (int k = 0; k < 8; k++) t->dec_bytes.push_back(0);
}

// added tokens (mod.rs:103-116 schema, :274-305 maps): content -> (id, flags) in file order, a
// later duplicate content replacing the earlier one; the special ones also into `special`
using AddedTokens = std::vector<std::pair<std::string, std::pair<uint32_t, uint8_t>>>;

AddedTokens parse_added_tokens(const ctj::Value* at, std::vector<std::pair<std::string, uint32_t>>& special_out) {
  AddedTokens added;
  if (!at) return added;
  if (at->kind != ctj::Value::Array) throw_err(CTOK_E_PARSE, "invalid type for `added_tokens`, expected a sequence");
  for (const auto& a : at->arr) {
    if (a.kind != ctj::Value::Object) throw_err(CTOK_E_PARSE, "invalid type: expected struct AddedToken");
    const ctj::Value* id = a.get("id");
    const ctj::Value* content = a.get("content");
    const ctj::Value* special = a.get("special");
    if (!id) throw_err(CTOK_E_PARSE, "missing field `id`");
    if (!content) throw_err(CTOK_E_PARSE, "missing field `content`");
    if (!special) throw_err(CTOK_E_PARSE, "missing field `special`");
    if (!id->is_u32()) throw_err(CTOK_E_PARSE, "invalid type for added token `id`, expected u32");
    if (content->kind != ctj::Value::String) throw_err(CTOK_E_PARSE, "invalid type for added token `content`, expected a string");
    if (special->kind != ctj::Value::Bool) throw_err(CTOK_E_PARSE, "invalid type for added token `special`, expected a boolean");
    uint8_t flags = (get_bool_field(a, "single_word", false, "AddedToken") ? 1 : 0) |
                    (get_bool_field(a, "lstrip", false, "AddedToken") ? 2 : 0) |
                    (get_bool_field(a, "rstrip", false, "AddedToken") ? 4 : 0);
    (void)get_bool_field(a, "normalized", false, "AddedToken");
    bool replaced = false;
    for (auto& e : added)
      if (e.first == content->s) { e.second = {(uint32_t)id->u, flags}; replaced = true; }
    if (!replaced) added.push_back({content->s, {(uint32_t)id->u, flags}});
    if (special->b) {
      bool rep = false;
      for (auto& e : special_out)
        if (e.first == content->s) { e.second = (uint32_t)id->u; rep = true; }
      if (!rep) special_out.push_back({content->s, (uint32_t)id->u});
    }
  }
  return added;
}

// The added tokens that can match inside a byte-mapped word, as raw-byte patterns (at_*), and
// with them whether every id encode can emit fits 16 bits (ids16; after compile_tables: narrow)
void compile_added_patterns(const AddedTokens& added, CompiledTables& t) {
  const std::vector<int> inv = byte_unmap();
  std::vector<uint32_t> cps;
  std::string raw;
  for (const auto& e : added) {
    if (e.first.empty()) throw_err(CTOK_E_UNSUPPORTED, "added token with empty content: the reference's word loop never terminates (src/huggingface/mod.rs:569-610)");
    if (!decode_utf8(e.first, cps) || !unmap_bytes(inv, cps, raw)) continue;
    if (!can_occur_in_piece(raw)) continue;  // provably never matches inside a piece
    t.at_bytes += raw;
    t.at_off.push_back((uint32_t)t.at_bytes.size());
    t.at_id.push_back(e.second.first);
    t.at_flags.push_back(e.second.second);
  }
  t.ids16 = t.narrow;
  for (uint32_t id : t.at_id) t.ids16 = t.ids16 && id < 0xFFFFu;
}

// add_prefix_space of the pre-tokenizer's one ByteLevel
bool parse_byte_level(const ctj::Value* v) {
  std::vector<std::pair<char, bool>> chain;
  parse_pre_tokenizer(v, chain, 0);
  int nbl = 0;
  bool add_prefix_space = false;
  for (auto& c : chain)
    if (c.first == 'B') { nbl++; add_prefix_space = c.second; }
  if (nbl != 1) throw_err(CTOK_E_UNSUPPORTED, "pre_tokenizer must contain exactly one ByteLevel");
  return add_prefix_space;
}

void load(ctok* t, const char* buf, size_t len) {
  const LoadKnobs knobs;
  LoadTimer timer{knobs.load_timing};
  ctj::Value root;
  try {
    root = ctj::parse(buf, len);
  } catch (const ctj::ParseError& e) {
    throw_err(CTOK_E_PARSE, e.what());
  }
  timer.lap("json");
  load_root(t, root, knobs.tables, timer);
}

// The tokenizer from its parsed tokenizer.json value (from a file, a buffer, or built from tables
// by ctok_create_from_tables).
void load_root(ctok* t, const ctj::Value& root, const TableOptions& opt, LoadTimer& timer) {
  if (root.kind != ctj::Value::Object) throw_err(CTOK_E_PARSE, "invalid type: expected struct TokenizerJson");
  const ctj::Value* model = root.get("model");
  if (!model) throw_err(CTOK_E_PARSE, "missing field `model`");
  if (model->kind != ctj::Value::Object) throw_err(CTOK_E_PARSE, "invalid type for `model`, expected struct ModelJson");
  const BpeModel m = parse_model(*model, t->vocab, t->id_to_token, timer);
  compile_tables(m, opt, *t, timer);
  compile_added_patterns(parse_added_tokens(root.get("added_tokens"), t->special), *t);
  t->nfc = parse_normalizer(root.get("normalizer")) != 0;
  t->add_prefix_space = parse_byte_level(root.get("pre_tokenizer"));
  parse_post_processor(t, root.get("post_processor"));
  t->decoder = parse_decoder(root.get("decoder"), t->decoder_name);
  build_decode_table(t);
  timer.lap("rest");
}


}  // namespace ctok_rt

using namespace ctok_rt;

extern "C" {

int ctok_create_from_buffer(const char* json, size_t len, ctok** out) {
  if (!out || (!json && len)) return fail(CTOK_E_ARG, "null argument");
  *out = nullptr;
  return run([&] {
    std::unique_ptr<ctok> t(new ctok());
    load(t.get(), json, len);
    *out = t.release();
  });
}

int ctok_create_from_tables(const ctok_tables* tb, ctok** out) {
  if (!tb || !out) return fail(CTOK_E_ARG, "null argument");
  *out = nullptr;
  return run([&] {
    if ((tb->n_vocab && (!tb->vocab || !tb->vocab_off || !tb->vocab_id)) ||
        (tb->n_merges && (!tb->merge_left || !tb->merge_right)) ||
        (tb->n_added && (!tb->added || !tb->added_off || !tb->added_id || !tb->added_flags)))
      throw_err(CTOK_E_ARG, "null table");
    // the value tree tokenizer.json would parse to (no JSON text): model.vocab, model.merges as
    // "a b" strings of the vocab's tokens, added_tokens, normalizer, ByteLevel pre-tokenizer/decoder
    auto str = [](std::string v) { ctj::Value x; x.kind = ctj::Value::String; x.s = std::move(v); return x; };
    auto num = [](uint64_t v) { ctj::Value x; x.kind = ctj::Value::Int; x.u = v; return x; };
    auto boo = [](bool v) { ctj::Value x; x.kind = ctj::Value::Bool; x.b = v; return x; };
    auto obj = [] { ctj::Value x; x.kind = ctj::Value::Object; return x; };
    ctj::Value vocab = obj(), merges, added;
    merges.kind = added.kind = ctj::Value::Array;
    std::unordered_map<uint32_t, std::string> by_id;
    vocab.obj.reserve(tb->n_vocab);
    for (uint64_t i = 0; i < tb->n_vocab; i++) {
      std::string k(tb->vocab + tb->vocab_off[i], tb->vocab_off[i + 1] - tb->vocab_off[i]);
      by_id[tb->vocab_id[i]] = k;
      vocab.obj.emplace_back(std::move(k), num(tb->vocab_id[i]));
    }
    merges.arr.reserve(tb->n_merges);
    for (uint64_t r = 0; r < tb->n_merges; r++) {
      auto a = by_id.find(tb->merge_left[r]), b = by_id.find(tb->merge_right[r]);
      if (a == by_id.end() || b == by_id.end())
        throw_err(CTOK_E_ARG, "merge " + std::to_string(r) + " names an id that is not in the vocab");
      // the reference joins every merge to "a b" and keeps it only when it splits on ' ' into
      // exactly two parts (src/huggingface/mod.rs:252-264, array form :87-94): a token holding a
      // space would be dropped silently and shift every later rank, so the table is refused
      if (a->second.find(' ') != std::string::npos || b->second.find(' ') != std::string::npos)
        throw_err(CTOK_E_ARG, "merge " + std::to_string(r) +
                                  " joins a token that contains ' ': the reference's merge format cannot express it");
      merges.arr.push_back(str(a->second + " " + b->second));
    }
    for (uint64_t i = 0; i < tb->n_added; i++) {
      ctj::Value e = obj();
      const uint8_t f = tb->added_flags[i];
      e.obj.emplace_back("id", num(tb->added_id[i]));
      e.obj.emplace_back("content", str(std::string(tb->added + tb->added_off[i], tb->added_off[i + 1] - tb->added_off[i])));
      e.obj.emplace_back("special", boo(f & CTOK_ADDED_SPECIAL));
      e.obj.emplace_back("single_word", boo(f & CTOK_ADDED_SINGLE_WORD));
      e.obj.emplace_back("lstrip", boo(f & CTOK_ADDED_LSTRIP));
      e.obj.emplace_back("rstrip", boo(f & CTOK_ADDED_RSTRIP));
      e.obj.emplace_back("normalized", boo(f & CTOK_ADDED_NORMALIZED));
      added.arr.push_back(std::move(e));
    }
    ctj::Value model = obj(), root = obj(), norm = obj(), pre = obj(), dec = obj();
    model.obj.emplace_back("type", str("BPE"));
    model.obj.emplace_back("vocab", std::move(vocab));
    model.obj.emplace_back("merges", std::move(merges));
    if (tb->nfc) {
      norm.obj.emplace_back("type", str("NFC"));
    } else {  // no normalisation (a null normalizer would mean NFC, src/huggingface/parsing.rs:89)
      ctj::Value none;
      none.kind = ctj::Value::Array;
      norm.obj.emplace_back("type", str("Sequence"));
      norm.obj.emplace_back("normalizers", std::move(none));
    }
    pre.obj.emplace_back("type", str("ByteLevel"));
    pre.obj.emplace_back("add_prefix_space", boo(tb->add_prefix_space != 0));
    dec.obj.emplace_back("type", str("ByteLevel"));
    root.obj.emplace_back("model", std::move(model));
    root.obj.emplace_back("added_tokens", std::move(added));
    root.obj.emplace_back("normalizer", std::move(norm));
    root.obj.emplace_back("pre_tokenizer", std::move(pre));
    root.obj.emplace_back("decoder", std::move(dec));
    auto t = std::make_unique<ctok>();
    const LoadKnobs knobs;
    LoadTimer timer{knobs.load_timing};
    load_root(t.get(), root, knobs.tables, timer);
    *out = t.release();
  });
}

int ctok_create_from_file(const char* path, ctok** out) {
  if (!path || !out) return fail(CTOK_E_ARG, "null argument");
  *out = nullptr;
  std::ifstream f(path, std::ios::binary);
  if (!f) return fail(CTOK_E_IO, std::string("No such file or directory (os error 2): ") + path);
  std::stringstream ss;
  ss << f.rdbuf();
  if (f.bad()) return fail(CTOK_E_IO, std::string("read error: ") + path);
  std::string s = ss.str();
  return ctok_create_from_buffer(s.data(), s.size(), out);
}

void ctok_destroy(ctok* t) { delete t; }

uint64_t ctok_vocab_size(const ctok* t) { return t ? t->vocab.size() : 0; }

int ctok_token_to_id(const ctok* t, const char* tok, size_t len, uint32_t* id) {
  if (!t || (!tok && len) || !id) return fail(CTOK_E_ARG, "null argument");
  auto it = t->vocab.find(std::string(tok, len));
  if (it == t->vocab.end()) return CTOK_E_NOTFOUND;
  *id = it->second;
  return CTOK_OK;
}

int ctok_id_to_token(const ctok* t, uint32_t id, char* buf, size_t cap, size_t* len) {
  if (!t || !len) return fail(CTOK_E_ARG, "null argument");
  auto it = t->id_to_token.find(id);
  if (it == t->id_to_token.end()) return CTOK_E_NOTFOUND;
  *len = it->second.size();
  if (buf && cap) memcpy(buf, it->second.data(), std::min(cap, it->second.size()));
  return CTOK_OK;
}

uint64_t ctok_num_special_tokens(const ctok* t) { return t ? t->special.size() : 0; }

int ctok_special_token(const ctok* t, uint64_t i, char* buf, size_t cap, size_t* len, uint32_t* id) {
  if (!t || !len || !id) return fail(CTOK_E_ARG, "null argument");
  if (i >= t->special.size()) return fail(CTOK_E_ARG, "index out of range");
  const auto& e = t->special[i];
  *len = e.first.size();
  *id = e.second;
  if (buf && cap) memcpy(buf, e.first.data(), std::min(cap, e.first.size()));
  return CTOK_OK;
}

uint64_t ctok_num_piece_added_tokens(const ctok* t) { return t ? t->at_id.size() : 0; }

int ctok_piece_can_contain(const uint8_t* raw, size_t len) {
  if (!raw && len) return fail(CTOK_E_ARG, "null argument");
  return can_occur_in_piece(std::string((const char*)raw, len)) ? 1 : 0;
}

uint64_t ctok_ids_bound(const ctok*, uint64_t n_bytes, uint64_t n_docs) { return 3 * n_bytes + n_docs + 16; }

uint64_t ctok_model_max_length(const ctok* t) { return t ? t->model_max_length : 0; }

int ctok_post_processor(const ctok* t, uint32_t* items, uint64_t cap, int64_t* n_items) {
  if (!t || !n_items) return fail(CTOK_E_ARG, "null argument");
  if (!t->has_pp) {
    *n_items = -1;
    return CTOK_OK;
  }
  *n_items = (int64_t)t->pp_items.size();
  for (uint64_t i = 0; i < t->pp_items.size() && i < cap && items; i++) items[i] = t->pp_items[i];
  return CTOK_OK;
}

// pad id: special_tokens["[PAD]"], else ["<pad>"], else 0 (src/huggingface/mod.rs:500-504)
uint32_t ctok_pad_id(const ctok* t) {
  if (!t) return 0;
  for (const char* name : {"[PAD]", "<pad>"})
    for (const auto& e : t->special)
      if (e.first == name) return e.second;
  return 0;
}

// src/huggingface/mod.rs:915-932
uint64_t ctok_num_special_tokens_to_add(const ctok* t, int is_pair) {
  if (!t) return 0;
  if (t->pp_kind == 3) return is_pair ? 3 : 2;
  if (t->pp_kind == 2) return is_pair ? 4 : 2;
  if (t->pp_kind != 1) return 0;
  const std::string& tpl = (is_pair && t->pp_has_pair) ? t->pp_pair : t->pp_single;
  std::vector<uint32_t> ch;
  if (!decode_utf8(tpl, ch)) return 0;
  uint64_t n = 0;
  size_t i = 0;
  while (i < ch.size()) {  // split_whitespace, parts not starting with '$'
    while (i < ch.size() && is_white_space(ch[i])) i++;
    if (i >= ch.size()) break;
    if (ch[i] != '$') n++;
    while (i < ch.size() && !is_white_space(ch[i])) i++;
  }
  return n;
}

}  // extern "C"
