// A Normalizer's program: the steps of include/ctok_normalizer.h expanded into the primitive steps
// of normalize_hd.h.  Shared by the host runtime (normalize_host.cpp) and the CPU check
// (tools/normalize_check.cpp).  Host-only; not part of the C ABI.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ctok_normalizer.h"
#include "normalize_hd.h"

namespace normalize {

struct PrimStep {
  uint32_t kind;  // Prim
  std::string a, b;
};

inline const char* prim_name(uint32_t kind) {
  static const char* names[] = {"decompose",       "decompose_compat", "reorder", "compose", "compose_compat",
                                "filter_accents",  "clean_text",       "chinese", "strip",   "replace",
                                "insert",          "prepend",          "append",  "lowercase"};
  return kind < sizeof(names) / sizeof(names[0]) ? names[kind] : "?";
}

inline void add_replace(std::vector<PrimStep>& out, const std::string& from, const std::string& to) {
  if (from.empty()) {
    if (!to.empty()) out.push_back({P_INSERT, "", to});
  } else if (from != to) {
    out.push_back({P_REPLACE, from, to});
  }
}

// The primitive steps of one step, appended to out; an error text, or null.
inline const char* expand(uint32_t kind, uint32_t flags, const std::string& a, const std::string& b,
                          std::vector<PrimStep>& out) {
  if (a.size() >= (1ull << 32) || b.size() >= (1ull << 32)) return "a step's string reaches 4 GiB";
  switch (kind) {
    case CTOK_NORM_NFC:
      out.insert(out.end(), {{P_DECOMP_D, "", ""}, {P_REORDER, "", ""}, {P_COMPOSE_C, "", ""}});
      return nullptr;
    case CTOK_NORM_NFD:
      out.insert(out.end(), {{P_DECOMP_D, "", ""}, {P_REORDER, "", ""}});
      return nullptr;
    case CTOK_NORM_NFKC:
      out.insert(out.end(), {{P_DECOMP_K, "", ""}, {P_REORDER, "", ""}, {P_COMPOSE_KC, "", ""}});
      return nullptr;
    case CTOK_NORM_NFKD:
      out.insert(out.end(), {{P_DECOMP_K, "", ""}, {P_REORDER, "", ""}});
      return nullptr;
    case CTOK_NORM_LOWERCASE:
      out.push_back({P_LOWER, "", ""});
      return nullptr;
    case CTOK_NORM_STRIP:
      out.push_back({P_STRIP, "", ""});
      return nullptr;
    case CTOK_NORM_STRIP_ACCENTS:
      out.insert(out.end(), {{P_DECOMP_D, "", ""}, {P_REORDER, "", ""}, {P_FILTER, "", ""}});
      return nullptr;
    case CTOK_NORM_REPLACE:
      add_replace(out, a, b);
      return nullptr;
    case CTOK_NORM_PREPEND:
      if (!a.empty()) out.push_back({P_PREPEND, a, ""});
      return nullptr;
    case CTOK_NORM_APPEND:
      if (!a.empty()) out.push_back({P_APPEND, a, ""});
      return nullptr;
    case CTOK_NORM_BERT: {  // src/normalizers.rs:59-92, in its order
      if (flags & CTOK_NORM_BERT_CLEAN_TEXT) out.push_back({P_CLEAN, "", ""});
      if (flags & CTOK_NORM_BERT_CHINESE) out.push_back({P_CHINESE, "", ""});
      expand(CTOK_NORM_NFC, 0, "", "", out);
      const bool lower = flags & CTOK_NORM_BERT_LOWERCASE;
      const bool strip = flags & CTOK_NORM_BERT_STRIP_ACCENTS_TRUE    ? true
                         : flags & CTOK_NORM_BERT_STRIP_ACCENTS_FALSE ? false
                                                                      : lower;
      if (strip) expand(CTOK_NORM_STRIP_ACCENTS, 0, "", "", out);
      if (lower) out.push_back({P_LOWER, "", ""});
      return nullptr;
    }
    case CTOK_NORM_PRECOMPILED: {  // one Replace per entry, in list order (:179-185)
      size_t p = 0;
      while (p < a.size()) {
        if (a.size() - p < 8) return "precompiled charsmap: a truncated entry";
        uint32_t nf, nt;
        memcpy(&nf, a.data() + p, 4);
        memcpy(&nt, a.data() + p + 4, 4);
        p += 8;
        if ((uint64_t)nf + nt > a.size() - p) return "precompiled charsmap: a truncated entry";
        add_replace(out, a.substr(p, nf), a.substr(p + nf, nt));
        p += (size_t)nf + nt;
      }
      return nullptr;
    }
    default:
      return "unknown normalizer step";
  }
}

}  // namespace normalize
