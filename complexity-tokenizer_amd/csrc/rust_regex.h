// Which patterns the Rust regex crate refuses to compile (ctok_load.cpp; restated in
// oracle/rust_regex.py): the reason, or "" for a pattern it compiles.  Shared by the loader and the
// PreTokenizer's `split` (pretok_host.cpp).  Not part of the C ABI.
#pragma once
#include <string>

namespace ctok_rt __attribute__((visibility("hidden"))) {
std::string rust_regex_rejects(const std::string& p);
}  // namespace ctok_rt
