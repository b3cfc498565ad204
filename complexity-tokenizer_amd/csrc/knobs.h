// Every CTOK_* environment variable the library reads, gathered by the time it is read.
// Host-only.  (The INL trainer's own variables are in trainer_host.cpp.)
#pragma once
#include <cstdint>
#include <cstdlib>
#include <optional>

#include "chunk_sort_hd.h"
#include "ctok_internal.h"
#include "table_compile.h"

namespace ctok_rt __attribute__((visibility("hidden"))) {

inline bool env_set(const char* name) { return getenv(name) != nullptr; }
inline int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}
inline std::optional<uint64_t> env_u64(const char* name) {
  const char* v = getenv(name);
  return v ? std::optional<uint64_t>(strtoull(v, nullptr, 10)) : std::nullopt;
}

// Read once per load (load, ctok_create_from_tables): the timing switch and the A/B arms of the
// table compiler (TableOptions, table_compile.h, which holds their defaults)
struct LoadKnobs {
  bool load_timing = env_set("CTOK_LOAD_TIMING");
  TableOptions tables = [] {
    TableOptions o;
    o.force_wide = env_set("CTOK_FORCE_WIDE");
    o.no_hot_table = env_set("CTOK_NO_HOT_TABLE");
    o.no_window = env_set("CTOK_NO_WINDOW");
    o.no_piece_table = env_set("CTOK_NO_PIECE_TABLE");
    o.merge_slack = (size_t)env_int("CTOK_MERGE_SLACK", (int)o.merge_slack);
    o.merge16_slack = (size_t)env_int("CTOK_MERGE16_SLACK", (int)o.merge16_slack);
    o.piece_slack = (size_t)env_int("CTOK_PIECE_SLACK", (int)o.piece_slack);
    return o;
  }();
};

// Read when the tables are uploaded to a device (device_state): what Tables says of them
struct UploadKnobs {
  bool force_improper = env_set("CTOK_FORCE_IMPROPER");
  bool force_wide_slots = env_set("CTOK_FORCE_WIDE_SLOTS");
  int short_packed = env_int("CTOK_SHORT_PACKED", 1);   // 0: the 16 + 16 register tier on every table
  int mid_packed = env_int("CTOK_MID_PACKED", ctok_dev::kMidPackedDefault);  // Tables::mid_packed
  uint32_t dbg_mode = (uint32_t)env_int("CTOK_DBG_MODE", 0);
};

// Read once per process, at the first use
struct ProcessKnobs {
  bool no_cp_ranges = env_set("CTOK_NO_CP_RANGES");
  bool debug_sync = env_set("CTOK_DEBUG_SYNC");
  bool safe_capacities = env_set("CTOK_SAFE_CAPACITIES");
  bool hostprof = env_set("CTOK_HOSTPROF");
  uint32_t unit = (uint32_t)env_int("CTOK_UNIT", 0);
  bool rec32 = env_set("CTOK_REC32");
  bool wgrec = env_set("CTOK_WGREC");
  bool stamps = env_set("CTOK_STAMPS");
  bool copy_results = env_set("CTOK_COPY_RESULTS");
  bool no_chunk_ramp = env_set("CTOK_NO_CHUNK_RAMP");
  bool pipe_trace = env_set("CTOK_PIPE_TRACE");
};
inline const ProcessKnobs& process_knobs() {
  static const ProcessKnobs k;
  return k;
}

// Read by every encode call (the tests flip C3_SPARSE, NFC_RERUN and WIRE32 within one process)
struct CallKnobs {
  bool no_nfc_speculation = env_set("CTOK_NO_NFC_SPECULATION");
  bool nfc_rerun = env_set("CTOK_NFC_RERUN");
  uint32_t short_wgs = (uint32_t)env_int("CTOK_SHORT_WGS", 0);
  // the merge passes' chunk order, the A/B arms of chunk_sort_hd.h (per call: the tests run every value in one process)
  uint32_t chunk_sort = (uint32_t)env_int("CTOK_CHUNK_SORT", (int)csort::kModeDefault) & csort::kModeMask;
  std::optional<uint64_t> c3_sparse = env_u64("CTOK_C3_SPARSE");  // the sparse class-3 bound (unset: the default rule)
  bool mid512 = env_set("CTOK_MID512");
  int overlap = env_int("CTOK_OVERLAP", ctok_dev::kOverlapDefault);  // >= 1: merge passes on the idle side stream
  bool wire32 = env_set("CTOK_WIRE32");
};

// Read by every training call of the classic BPE trainer (bpe_train_host.cpp; the tests flip them
// within one process).  Its counting also reads the INL trainer's CTOK_TRAIN_CHUNK_BYTES and
// CTOK_TRAIN_COUNT_SLOTS.
struct BpeTrainKnobs {
  std::optional<uint64_t> slots = env_u64("CTOK_BPE_TRAIN_SLOTS");  // cap of the pair table's capacity
  bool recount = env_int("CTOK_BPE_TRAIN_RECOUNT", 0) != 0;         // count all pairs again before every merge
};

// Read by every training call of the WordPiece trainer (wordpiece_host.cpp).  Its pair table also
// reads BpeTrainKnobs::slots, its counting CTOK_TRAIN_CHUNK_BYTES and CTOK_TRAIN_COUNT_SLOTS.
struct WpTrainKnobs {
  bool recount = env_int("CTOK_WP_TRAIN_RECOUNT", 0) != 0;  // walk every word and count all pairs again in every round
};

// Read when a PreTokenizer handle is made and by ctok_pretok_limits (pretok_host.cpp).  A `split`
// pattern that runs as a cyclic DFA costs a matching run of R code points about R * R / 2 steps, so a
// start may step through at most kMaxRegexRun code points (the largest power of two
// at which the worst case finishes within about 2 s).  The variable lowers the cap; nothing raises it.
constexpr uint32_t kMaxRegexRun = 1u << 19;
struct PretokKnobs {
  uint32_t max_regex_run = [] {
    uint64_t cap = kMaxRegexRun;
    if (auto e = env_u64("CTOK_PRETOK_MAX_REGEX_RUN")) cap = *e < cap ? *e : cap;
    return (uint32_t)cap;
  }();
};

}  // namespace ctok_rt
