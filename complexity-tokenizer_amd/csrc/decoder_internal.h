// What the Decoder's host runtime (decoder_host.cpp) calls in decoder.hip, and how a step of
// include/ctok_decoder.h becomes ops (also tools/decoder_check.cpp's).  Not part of the C ABI.
// Every pointer of the launch functions is a device pointer (a Step's strings too).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "decoder_hd.h"

namespace decoder {

enum Kind : uint32_t { K_BYTE_LEVEL, K_METASPACE, K_WORDPIECE, K_BPE, K_CTC, K_FUSE, K_STRIP, K_REPLACE, K_N };  // ctok_decoder.h

inline const char* kind_name(uint32_t k) {
  static const char* const names[] = {"byte_level", "metaspace", "wordpiece", "bpe", "ctc", "fuse", "strip", "replace"};
  return k < K_N ? names[k] : "?";
}

// what an op does before its units are counted
enum Prep : uint32_t { P_NONE, P_STRIP, P_TRIM, P_WP_FIRST, P_REPLACE, P_CLEANUP };

struct HostOp {
  uint32_t op, flags, prep;
  std::string a, b;
  uint64_t start, stop;
};

inline std::string utf8_of_cp(uint32_t c) {
  std::string s;
  if (c < 0x80) s += (char)c;
  else if (c < 0x800) { s += (char)(0xC0 | (c >> 6)); s += (char)(0x80 | (c & 63)); }
  else if (c < 0x10000) { s += (char)(0xE0 | (c >> 12)); s += (char)(0x80 | ((c >> 6) & 63)); s += (char)(0x80 | (c & 63)); }
  else { s += (char)(0xF0 | (c >> 18)); s += (char)(0x80 | ((c >> 12) & 63)); s += (char)(0x80 | ((c >> 6) & 63)); s += (char)(0x80 | (c & 63)); }
  return s;
}

// The ops of one step, appended to out; an error text when the step is not one (bad kind or code point).
inline const char* expand(uint32_t kind, uint32_t flags, const std::string& a, const std::string& b, uint32_t cp, uint64_t start,
                          uint64_t stop, std::vector<HostOp>* out) {
  const bool is_char = cp < 0x110000 && !(cp >= 0xD800 && cp < 0xE000);
  switch (kind) {
    case K_BYTE_LEVEL:
      out->push_back(HostOp{OP_BL_MAP, 0, P_NONE, "", "", 0, 0});
      out->push_back(HostOp{OP_LOSSY, 0, P_NONE, "", "", 0, 0});
      return nullptr;
    case K_METASPACE:
      if (!is_char) return "the replacement is no code point";
      out->push_back(HostOp{OP_METASPACE, flags & 1u, P_NONE, utf8_of_cp(cp), "", 0, 0});
      return nullptr;
    case K_WORDPIECE:
      out->push_back(HostOp{OP_WORDPIECE, 0, P_WP_FIRST, a, "", 0, 0});
      if (flags & 1u) out->push_back(HostOp{OP_DEAD, 0, P_CLEANUP, "", "", 0, 0});
      return nullptr;
    case K_BPE:
      out->push_back(HostOp{OP_BPE, 0, P_NONE, a, "", 0, 0});
      out->push_back(HostOp{OP_RANGE, 0, P_TRIM, "", "", 0, 0});
      return nullptr;
    case K_CTC:
      out->push_back(HostOp{OP_CTC, flags & 1u, P_NONE, a, (flags & 1u) ? b : std::string(), 0, 0});
      return nullptr;
    case K_FUSE:
      out->push_back(HostOp{OP_FUSE, 0, P_NONE, "", "", 0, 0});
      return nullptr;
    case K_STRIP:
      if (!is_char) return "the content is no code point";
      out->push_back(HostOp{OP_RANGE, 0, P_STRIP, utf8_of_cp(cp), "", start, stop});
      return nullptr;
    case K_REPLACE:
      if (a.empty()) out->push_back(HostOp{OP_INSERT, 0, P_NONE, "", b, 0, 0});
      else out->push_back(HostOp{OP_MARK, 0, P_REPLACE, a, b, 0, 0});
      return nullptr;
    default:
      return "no such decoder";
  }
}

}  // namespace decoder

#if defined(__HIP_PLATFORM_AMD__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace ctok_dc {

constexpr uint32_t kThreads = 256;  // a workgroup, and the units of its tile: a thread owns one byte or one token

// blocks of an op over n units: the place behind the last unit is a unit that emits nothing, so that
// the documents that start there (the empty ones at the end, every one of an empty batch) have a block
inline uint64_t unit_blocks(uint64_t n_units) { return (n_units + 1 + kThreads - 1) / kThreads; }

// flag[0] |= 1 unless tok_off and doc_tok are in order: both start at 0 and do not decrease,
// doc_tok[n_docs] = n_tok, tok_off[n_tok] = n_bytes
hipError_t launch_check(const uint64_t* tok_off, uint64_t n_tok, uint64_t n_bytes, const uint64_t* doc_tok, uint64_t n_docs,
                        uint32_t* flag, hipStream_t s);
// doc_off[d] = tok_off[doc_tok[d]], d in [0, n_docs]
hipError_t launch_doc_off(const uint64_t* tok_off, const uint64_t* doc_tok, uint64_t n_docs, uint64_t* doc_off, hipStream_t s);
// p[i] = i, i in [0, n]
hipError_t launch_iota(uint64_t* p, uint64_t n, hipStream_t s);
// an op's preparation (prep of HostOp): lo / hi (n_docs), first (n_docs), cand / mark (n bytes; zeroed here)
struct Scratch {
  uint64_t* lo;
  uint64_t* hi;
  uint64_t* first;
  uint8_t* cand;
  uint8_t* mark;
};
hipError_t launch_prep(uint32_t prep, const decoder::Step& st, uint64_t start, uint64_t stop, const decoder::In& in,
                       const Scratch& sc, hipStream_t s);
// blk[i] = the bytes the units of block i emit (unit_blocks() entries, for scan_u64) ...
hipError_t launch_count(const decoder::Step& st, const decoder::In& in, uint64_t* blk, hipStream_t s);
// ... and after the scan: the bytes, the documents' new offsets (n_docs + 1) and their tails
hipError_t launch_write(const decoder::Step& st, const decoder::In& in, const uint64_t* blk, uint8_t* out, uint64_t* out_off,
                        hipStream_t s);

// The gather of the ids entry.  ent: (offset, length) per id, length CTOK_DEC_NO_ENTRY: none.
// keep[j] = 1 when ids[j] has an entry (n_ids + 1 entries, for scan_u64)
hipError_t launch_gather_keep(const uint32_t* ids, uint64_t n_ids, const uint2* ent, uint64_t n_ent, uint64_t* keep, hipStream_t s);
// len[pos[j]] = the bytes of kept id j (n_tok + 1 entries, for scan_u64); doc_tok[d] = pos[ids_off[d]]
hipError_t launch_gather_len(const uint32_t* ids, uint64_t n_ids, const uint2* ent, uint64_t n_ent, const uint64_t* pos,
                             const uint64_t* ids_off, uint64_t n_docs, uint64_t* len, uint64_t* doc_tok, hipStream_t s);
// the tokens' bytes at tok_off (len after its scan)
hipError_t launch_gather_write(const uint32_t* ids, uint64_t n_ids, const uint2* ent, uint64_t n_ent, const uint8_t* pool,
                               const uint64_t* pos, const uint64_t* tok_off, uint8_t* out, hipStream_t s);

}  // namespace ctok_dc
#endif
