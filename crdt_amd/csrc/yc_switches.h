// yc_switches.h — every YCRDT_* environment switch the C++ reads: one table, one reader.
//
// The switches force decode paths, turn the small-merge kernels off, shrink windows and serve as test
// hooks; all default to the measured-best setting. Nothing else under crdt_amd/csrc calls getenv.
// A row of YC_SWITCHES is X(type, field, name, parse, default, when, what):
//   parse(text, default) gives the field from the variable's text (nullptr: unset). The kinds:
//     sw_off  off-switch: false when the text starts with '0' ("0", "00", "0x"; not " 0", "", "false")
//     sw_on   on-switch: true when the text starts with '1' ("1", "10"; not "true", " 1")
//     sw_set  on when set at all, "" and "0" included
//     keyword a whole-word compare, anything else the default (sw_decode, sw_yata, sw_wdecode), some with
//             a first-character '0' / '1' beside it (sw_fwc, sw_predecode, sw_direct_wave, sw_spec_hint)
//     integer atoi / strtoull with the row's own range, out of range the default (sw_count, sw_positive,
//             sw_schunk, sw_win_shift, sw_hash_bits, sw_pin_chunk, pass_bytes of yc_engine_host.h)
//   when: the moment the variable is read; the answer then holds for
//     PROCESS  the process: process_switches(), read at its first use
//     ENGINE   the engine: read by ycrdt_engine_create
//     BATCH    the staged batch: ycrdt_batch::sw, read when the batch is staged (layout) and kept
//              through its merge, view, results, a generous re-run and a re-stage after a JSON rewrite
//     CALL     one call over many documents (ycrdt_docs_*, ycrdt_merge_updates_groups), read at entry
//   what: the effect, and who sets it (tests, A/B runs, experiments).
// INTEGRATION.md "Environment switches" lists the same rows (tests/test_switches.py compares the names).
// Builds with a plain C++ compiler (tests/csrc/switches_main.cpp runs the reader under the sanitizers).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "yc_engine_host.h"  // pass_bytes, JSON_PASS_BYTES

#pragma GCC visibility push(hidden)
namespace yc {

enum class DecodeMode : uint8_t { AUTO, CHUNKS, DIRECT, XTAB };  // XTAB: chunks, and every large update through the exit tables
enum class DirectWave : uint8_t { AUTO, LANE, WAVE };            // small updates: by their count / one lane each / one wavefront each
enum class FwcMode : uint8_t { ON, OFF, FORCE };
enum class Predecode : uint8_t { ON, OFF, CHECK };
enum class SpecHint : uint8_t { NEVER = 0, ALWAYS = 1, SINGLE_SECTION = 2 };  // (the values Work::spec_hint carries)
enum class YataMode : uint8_t { TREE, SEQ };
enum class WdecodeMode : uint8_t { RANK, SETTLE };

constexpr uint32_t SCHUNK_LIMIT = 1024;  // = SCHUNK of yc_common.h (a device header; asserted equal in yc_engine.hip)

inline bool sw_off(const char* v, bool d) { return v && v[0] == '0' ? false : d; }
inline bool sw_on(const char* v, bool d) { return v && v[0] == '1' ? true : d; }
inline bool sw_set(const char* v, bool) { return v != nullptr; }
inline DecodeMode sw_decode(const char* v, DecodeMode d) {  // ("tables": the older name of "chunks")
  if (!v) return d;
  return !strcmp(v, "chunks") || !strcmp(v, "tables") ? DecodeMode::CHUNKS : !strcmp(v, "xtab") ? DecodeMode::XTAB
         : !strcmp(v, "direct") ? DecodeMode::DIRECT : d;
}
inline DirectWave sw_direct_wave(const char* v, DirectWave d) { return v && v[0] == '0' ? DirectWave::LANE : v && v[0] == '1' ? DirectWave::WAVE : d; }
inline FwcMode sw_fwc(const char* v, FwcMode d) { return v && v[0] == '0' ? FwcMode::OFF : v && !strcmp(v, "force") ? FwcMode::FORCE : d; }
inline Predecode sw_predecode(const char* v, Predecode d) { return v && v[0] == '0' ? Predecode::OFF : v && !strcmp(v, "check") ? Predecode::CHECK : d; }
inline SpecHint sw_spec_hint(const char* v, SpecHint d) { return v && v[0] == '1' ? SpecHint::ALWAYS : v && v[0] == '0' ? SpecHint::NEVER : d; }
inline YataMode sw_yata(const char* v, YataMode d) { return v && !strcmp(v, "seq") ? YataMode::SEQ : d; }
inline WdecodeMode sw_wdecode(const char* v, WdecodeMode d) { return v && !strcmp(v, "settle") ? WdecodeMode::SETTLE : d; }
inline uint32_t sw_count(const char* v, uint32_t d) { return v ? (uint32_t)atoi(v) : d; }  // (any number, 0 and below included)
inline uint32_t sw_positive(const char* v, uint32_t d) { return v && atoi(v) > 0 ? (uint32_t)atoi(v) : d; }
inline uint32_t sw_schunk(const char* v, uint32_t d) {
  const uint32_t x = v ? (uint32_t)atoi(v) : 0;
  return x >= 64 && x <= SCHUNK_LIMIT && x % 64 == 0 ? x : d;
}
inline uint32_t sw_win_shift(const char* v, uint32_t d) {
  const int x = v ? atoi(v) : 0;
  return x >= 16 && x <= 32 ? (uint32_t)x : d;
}
inline uint32_t sw_hash_bits(const char* v, uint32_t d) {
  const int x = v ? atoi(v) : 0;
  return x >= 1 && x < 64 ? (uint32_t)x : d;
}
inline uint64_t sw_pin_chunk(const char* v, uint64_t d) {
  const uint64_t c = v ? strtoull(v, nullptr, 10) : 0;
  return c >= 4096 && c <= (uint64_t(1) << 30) ? c : d;
}

// clang-format off
#define YC_SWITCHES(X) \
  /* ---- staging (layout) */ \
  X(DecodeMode, decode, "YCRDT_DECODE", sw_decode, DecodeMode::AUTO, BATCH, "chunks|tables|direct: one decoder for the small updates; xtab: chunks, and large updates through the exit tables. A typo forces nothing. Parity tests run every one") \
  X(DirectWave, direct_wave, "YCRDT_DIRECT_WAVE", sw_direct_wave, DirectWave::AUTO, BATCH, "first character 0: small updates one lane each (few of them then take the chunk path); 1: one wavefront each. Tests") \
  X(FwcMode, fwc, "YCRDT_FWC", sw_fwc, FwcMode::ON, BATCH, "first character 0: record mode of the multi-section fast walk off; the word force: for every large update of two or more sections. Tests, A/B") \
  X(uint32_t, schunk, "YCRDT_SCHUNK", sw_schunk, 0u, BATCH, "a fixed chunk size: a multiple of 64 in [64, SCHUNK], anything else (0) leaves the choice to the batch. Experiments") \
  X(uint32_t, win_shift, "YCRDT_WIN_SHIFT", sw_win_shift, 32u, BATCH, "byte windows of 2^n, n in [16, 32]: every multi-window path on a few MB. Tests") \
  X(uint64_t, pin_chunk, "YCRDT_PIN_CHUNK", sw_pin_chunk, uint64_t(32) << 20, BATCH, "bytes of a pinned staging chunk, in [4096, 2^30]: the two-half wave path on small batches (the calls over many documents: CALL). Tests") \
  X(Predecode, predecode, "YCRDT_PREDECODE", sw_predecode, Predecode::ON, BATCH, "first character 0: a doc state is decoded again, not from its encode's marks; the word check: both, compared word by word. Tests") \
  /* ---- decode */ \
  X(bool, prewalk, "YCRDT_PREWALK", sw_off, true, BATCH, "0: no exact pre-walk of large updates with a short struct section. A/B") \
  X(bool, walk_only, "YCRDT_WALK_ONLY", sw_off, true, BATCH, "0: the chunk walk runs even when the pre-walk takes every large update. A/B") \
  X(bool, no_fastwalk, "YCRDT_NO_FASTWALK", sw_on, false, BATCH, "1: k_walk alone, without the fast walks. Tests compare the two") \
  X(WdecodeMode, wdecode, "YCRDT_WDECODE", sw_wdecode, WdecodeMode::RANK, BATCH, "settle: the wavefront-per-update chains of k_wdecode instead of the ranking. Tests") \
  X(SpecHint, spec_hint, "YCRDT_SPEC_HINT", sw_spec_hint, SpecHint::SINGLE_SECTION, BATCH, "chunk-start hints, first character 1 / 0: always / never (default: single-section updates only). Experiments") \
  X(uint32_t, fwm_max, "YCRDT_FWM_MAX", sw_count, 0u, BATCH, "record mode vouches for at most n sections (atoi; unset and 0: no limit). Tests: the ranked path") \
  X(uint32_t, fwc_walk, "YCRDT_FWC_WALK", sw_positive, 256u, BATCH, "the record walker's step count, n > 0. Experiments") \
  X(bool, rtab, "YCRDT_RTAB", sw_off, true, BATCH, "0: record mode parses every step (no step table). A/B") \
  X(bool, rank_last, "YCRDT_RANK_LAST", sw_off, true, BATCH, "0: the last section the records left goes to k_walk, not the ranking. A/B") \
  X(uint32_t, test_section_cap, "YCRDT_TEST_SECTION_CAP", sw_positive, 0u, BATCH, "n > 0: a section estimate of at most n, forcing the overflow re-run (0: none). Tests") \
  X(bool, test_fail_before_exchange, "YCRDT_TEST_FAIL_BEFORE_EXCHANGE", sw_on, false, BATCH, "1: this rank fails on the host before a sharded merge's decode exchange. Test hook") \
  X(bool, decode_small, "YCRDT_DECODE_SMALL", sw_off, true, BATCH, "0: none of the decode's single-workgroup kernels. Tests, A/B") \
  X(bool, decode_quick, "YCRDT_DECODE_QUICK", sw_off, true, BATCH, "0: a small batch keeps its count synchronisation. Tests, A/B") \
  X(bool, ds_grid, "YCRDT_DS_GRID", sw_off, true, BATCH, "0: every delete set decoded on the wavefront. Tests compare the two") \
  X(bool, ds_jump, "YCRDT_DS_JUMP", sw_off, true, BATCH, "0: the lane-serial walk of the delete-set headers. A/B") \
  X(bool, sd_group, "YCRDT_SD_GROUP", sw_off, true, BATCH, "0: structs decoded without grouping a workgroup's structs by shape. A/B") \
  X(bool, scan_fused, "YCRDT_SCAN_FUSED", sw_off, true, BATCH, "0: the large batches' separate scan passes. A/B") \
  X(bool, debug_bounds, "YCRDT_DEBUG_BOUNDS", sw_on, false, BATCH, "1: every unit flag store, key slot and small-kernel index checked against its table (the diff arguments of ycrdt_docs_diff: CALL). Tests") \
  X(bool, debug_yata, "YCRDT_DEBUG_YATA", sw_on, false, BATCH, "1: the debug counters' buffer for the YATA kernels. Experiments") \
  X(bool, debug_decode, "YCRDT_DEBUG_DECODE", sw_on, false, BATCH, "1: why the fast walks left updates to k_walk, on stderr. Experiments") \
  /* ---- merge, encode, view */ \
  X(bool, ds_tails, "YCRDT_DS_TAILS", sw_off, true, BATCH, "0: a long delete-set run is flagged by the wavefront that met it. A/B") \
  X(uint32_t, key_hash_bits, "YCRDT_KEY_HASH_BITS", sw_hash_bits, 64u, BATCH, "n in [1, 63]: only the low n bits of every list hash (collisions certain); unset, 0 and the rest: all 64. Test hook") \
  X(bool, merge_small, "YCRDT_MERGE_SMALL", sw_off, true, BATCH, "0: no single-workgroup merge. Tests, A/B") \
  X(bool, phase_fence, "YCRDT_PHASE_FENCE", sw_on, false, BATCH, "1: agent-scope fences at every phase boundary of k_merge_small. Tests, A/B") \
  X(bool, yata_global, "YCRDT_YATA_GLOBAL", sw_set, false, BATCH, "set to anything, 0 included: the sequential YATA kernel without its LDS variants. Experiments") \
  X(bool, encode_small, "YCRDT_ENCODE_SMALL", sw_off, true, BATCH, "0: no single-workgroup encode. Tests, A/B") \
  X(bool, enc_record, "YCRDT_ENC_RECORD", sw_off, true, BATCH, "0: the encode without its per-struct record, every struct written from its columns. Tests, A/B") \
  X(bool, view_small, "YCRDT_VIEW_SMALL", sw_off, true, BATCH, "0: no single-workgroup view. Tests, A/B") \
  /* ---- the calls over many documents */ \
  X(bool, sync, "YCRDT_SYNC", sw_off, true, CALL, "0: ycrdt_docs_diff answers every pair by the single call. Tests") \
  X(bool, store, "YCRDT_STORE", sw_off, true, CALL, "0: ycrdt_merge_updates_groups merges every group by the single call. Tests") \
  X(bool, docs_json, "YCRDT_DOCS_JSON", sw_off, true, CALL, "0: ycrdt_docs_json by the single calls. Tests") \
  X(bool, docs_cache, "YCRDT_DOCS_CACHE", sw_off, true, CALL, "0: ycrdt_docs_cache by the single calls. Tests") \
  X(bool, docs_read, "YCRDT_DOCS_READ", sw_off, true, CALL, "0: ycrdt_docs_read by the single calls. Tests") \
  X(bool, docs_write, "YCRDT_DOCS_WRITE", sw_off, true, CALL, "0: ycrdt_docs_write by the single calls. Tests") \
  X(bool, docs_transact, "YCRDT_DOCS_TRANSACT", sw_off, true, CALL, "0: ycrdt_docs_transact by the single calls. Tests") \
  X(uint64_t, docs_json_pass_bytes, "YCRDT_DOCS_JSON_PASS_BYTES", pass_bytes, JSON_PASS_BYTES, CALL, "state bytes per device pass of ycrdt_docs_json (unset, 0 and above the cap: the cap). Tests: several passes on a few documents") \
  X(uint64_t, docs_cache_pass_bytes, "YCRDT_DOCS_CACHE_PASS_BYTES", pass_bytes, JSON_PASS_BYTES, CALL, "the same for ycrdt_docs_cache. Tests") \
  X(uint64_t, docs_read_pass_bytes, "YCRDT_DOCS_READ_PASS_BYTES", pass_bytes, JSON_PASS_BYTES, CALL, "the same for ycrdt_docs_read. Tests") \
  X(uint64_t, docs_write_pass_bytes, "YCRDT_DOCS_WRITE_PASS_BYTES", pass_bytes, JSON_PASS_BYTES, CALL, "the same for ycrdt_docs_write. Tests") \
  X(uint64_t, docs_transact_pass_bytes, "YCRDT_DOCS_TRANSACT_PASS_BYTES", pass_bytes, JSON_PASS_BYTES, CALL, "the same for ycrdt_docs_transact. Tests") \
  /* ---- once per engine, once per process */ \
  X(bool, debug_sync, "YCRDT_DEBUG_SYNC", sw_on, false, ENGINE, "1: synchronise after every phase, so a device fault is attributed to its phase. Experiments") \
  X(bool, rocprim_scan, "YCRDT_ROCPRIM_SCAN", sw_on, false, PROCESS, "1: rocPRIM's scans instead of the engine's own. Experiments") \
  X(YataMode, yata, "YCRDT_YATA", sw_yata, YataMode::TREE, PROCESS, "seq: the sequential YATA kernel instead of the tree. Tests (in a child process)") \
  X(bool, ylists_eager, "YCRDT_YLISTS_EAGER", sw_on, false, PROCESS, "1: the tree path numbers the lists at once, not when a view asks. A/B") \
  X(bool, view_sync, "YCRDT_VIEW_SYNC", sw_on, false, PROCESS, "1: a small view sizes its key copy first, as a large one does. A/B") \
  X(bool, no_fold, "YCRDT_NO_FOLD", sw_on, false, PROCESS, "1: a doc's merge copies its state out after the last synchronisation, not before. A/B")
// clang-format on

struct Switches {
#define X(type, field, name, parse, dflt, when, what) type field = dflt;
  YC_SWITCHES(X)
#undef X
};

// the environment as it is now
inline Switches read_switches() {
  Switches s;
#define X(type, field, name, parse, dflt, when, what) s.field = parse(getenv(name), dflt);
  YC_SWITCHES(X)
#undef X
  return s;
}

// the PROCESS rows (the other fields hold what the environment said at the first call: not for use)
inline const Switches& process_switches() {
  static const Switches s = read_switches();
  return s;
}

}  // namespace yc
#pragma GCC visibility pop
