// qmx_text.h — byte-level text primitives shared by the CPU engine and the CDNA4 kernels.
//
// Everything here is `__host__ __device__`: the host engine (qmx_cpu.cpp) and the fused
// tick/finalize kernels (qmx_hip.hip) call the SAME code for the per-event pieces
// (UTF-8 validation, Unicode whitespace, the validating JSON delta extractor, JSON
// string decode, ensure_ascii escape), so the two engines can only differ in the
// data-parallel parts (framing scan, MFMA tag match, depth scan, compaction), which
// the differential tests pin against each other and against the python oracle.
//
// Semantics = SURVEY §2.7 (reference src/quorum/oai_proxy.py:120-139, 262-371, 578-673).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qmx_unicode_classes.h"

#define QMX_HD __host__ __device__ inline

namespace qmx {

// Tag sets the native engines run exactly ("<= ~16 tags"): up to 16 distinct
// (lowercased) tags of up to 61 printable-ASCII bytes with no regex metacharacter and no
// '<', '>' or '/'.  The MFMA matcher compares a 16-byte window per candidate '<' (a pattern
// longer than that — "</" + tag + ">" beyond 16 bytes — is a window prefix match plus a
// compare of its tail bytes), 16 patterns per MFMA column block (open + close of 16 tags:
// two blocks).  The holdback of a partial tag is at most the longest pattern - 1 bytes.
constexpr int kMaxTags = 16;
constexpr int kMaxTagLen = 61;   // "</" + 61 + ">" = 64 bytes
constexpr int kWindow = 16;
constexpr int kMaxTail = 64;
// per-stream event shape template (qmx_lex.h): the longest prefix before the content string
// and suffix after it that are kept
constexpr int TPL_PRE_MAX = 256, TPL_SUF_MAX = 64, TPL_BYTES = TPL_PRE_MAX + TPL_SUF_MAX;
constexpr int kJsonMaxDepth = 256;  // deeper == RecursionError (stream abort)

// ---------------------------------------------------------------------------
// tag patterns
// ---------------------------------------------------------------------------
// The three kinds of tag set (host code keeps the kind with the tables: Tags, qmx_engine.h).
//   literal: ASCII or uncased tags, compared byte for byte (ASCII letters lowercased);
//   class:   some tag took the class parser (a class element or an escape);
//   pair:    literal tags with a cased non-ASCII character, the text folded as it is read;
//   mixed:   a class element and a non-ASCII literal character in one set (make_tags' `mixed`):
//            the class rules, the text folded as it is read.
enum TagKind : int { TAGS_LITERAL, TAGS_CLASS, TAGS_PAIR, TAGS_MIXED };

// Class tags (make_tags(tags, classes = true)): the fixed-width part of the regex language
// the reference's alternation speaks — '.', bracket classes and escaped punctuation.  A tag is
// then a sequence of elements that match one code point each; name[] keeps a literal element
// as its lowercase byte and a class element as 0x80 + its index into TagClasses (pattern bytes
// are otherwise printable ASCII), len[] counts elements.
constexpr int kMaxClasses = 32;
constexpr int kMaxFold = 32;  // distinct pair characters of a pair tag set
enum : uint8_t { CLS_WIDE = 1, CLS_DOT = 2 };  // accepts non-ASCII code points / is a '.'
// A class with a shorthand (make_tags(..., extended = true): \d, \w, \s, alone or in brackets) holds
// SOME code points >= 0x80: one bit per shorthand, tables in qmx_unicode_classes.h (host only).
// With such a bit CLS_WIDE says the class is negated: the answer is member XOR negated.  Read
// only where a class position holds a byte >= 0x80.
enum : uint8_t { CLS_SH_DIGIT = 4, CLS_SH_WORD = 8, CLS_SH_SPACE = 16, CLS_SH = 4 | 8 | 16 };
struct TagClasses {
  int n;                               // distinct class definitions
  uint32_t tab[kMaxClasses][4];        // ASCII acceptance under IGNORECASE | DOTALL (bit b of the 128)
  uint8_t flags[kMaxClasses];
  int srclen[kMaxTags];
  uint8_t src[kMaxTags][kMaxTagLen + 1];  // the tag's lowercased source text (depth-0 holdback)
  // Pair tag sets (make_tags(tags, classes, unicode = true), a non-ASCII cased character in
  // a tag): the tags are literal — n == 0, name[] holds the UTF-8 bytes of the lowercased tag —
  // and the text is folded as it is read: the upper member of a pair stands for its lower
  // member (same byte length).  A character's bytes are packed little-endian, byte k at bit 8k.
  int nfold;                           // distinct pair characters of the tags; 0: a class tag set; < 0: a mixed one
  int span;                            // bytes of the longest pattern
  uint8_t fold_len[kMaxFold];
  uint32_t fold_up[kMaxFold], fold_lo[kMaxFold];
  // Mixed tag sets (make_tags(..., mixed = true), a class element and a non-ASCII literal in one
  // set): name[] holds lowercase ASCII bytes, the UTF-8 bytes of the lowered non-ASCII literals
  // and one marker byte 0x80 + class index per class position; len[] counts those bytes.  A
  // marker is told from a UTF-8 byte by position: bit i of clsmask[t] — name[t][i] is a marker.
  // walk: bit t — tag t has a class element or a pair character (the byte matchers cannot
  // decide it).  n and the fold tables are as above; span is unused.  The kind rides in nfold,
  // the one word the kernels of the class kind read to choose their path: a mixed tag set with
  // k pair characters keeps -(k + 1) there (mixed_nfold), so a class or pair tag set's device
  // data, and the loads that decide its path, are what they were.
  uint32_t walk;
  uint64_t clsmask[kMaxTags];
  // Variable-width tags (make_tags(..., variants = true): '?', '|' and groups).  Such a tag is
  // kept as its rows — its fixed-width expansions in the regex's priority order, one entry of
  // TagSet each, src[] of every one the tag's whole source text.  var: bit r — row r comes from
  // such a tag; 0 for every other set.  The last field, read only where a class position holds
  // '<', '>' or a byte >= 0x80 (variant_mismatch): the other sets' data and loads are what they were.
  // Bits 0-15 are rows.  kVarExtended (make_tags(..., extended = true)): the set was made with
  // the extended language; the finalize of such a class set goes on to a tag's next close where
  // the first is not the open's captured text (`step\d`: <step1>a</step2>b</step1>).
  uint32_t var;
  // Unbounded repetition (make_tags(..., repeat = true): '+', '*', "{m,}" after one element).  Such
  // a quantifier expands as x{m, m + kRepeatRows - 1} does, and the longest row is open-ended at
  // its last copy of x: "this many or more".  rep[t]: bit i — position i of name[t] (always a class
  // position: the same convention as clsmask) is open-ended; 0 for every other row and set.  The last
  // field, read only at a class position that has matched.
  uint64_t rep[kMaxTags];
};
constexpr uint32_t kVarRows = 0xffffu, kVarExtended = 1u << 31;
// kVarRuns (make_tags(..., runs = true), a set with an open-ended row): the device walks take a run
// of ASCII copies past an open-ended row themselves (WALK_RUNS) instead of leaving it to the host.
constexpr uint32_t kVarRuns = 1u << 30;
// Rows an unbounded quantifier expands into beyond its minimum count: `x+` is the counts 4, 3, 2, 1
// (`x*`: and 0), `x{m,}` m+3 ... m.  Runs up to the longest row's count are decided by the rows (on
// the GPU); a longer run is decided by the exact host walk.
constexpr int kRepeatRows = 4;
// The kernels of the class kind run class, pair and mixed tag sets (KParams::cls is set for all
// three): which of them the tables are.
QMX_HD bool is_pair_set(const TagClasses& tc) { return tc.nfold > 0; }
QMX_HD bool is_mixed_set(const TagClasses& tc) { return tc.nfold < 0; }
QMX_HD int mixed_nfold(const TagClasses& tc) { return -tc.nfold - 1; }  // pair characters of a mixed tag set

// (The layout of TagSet is the literal tag sets': the kernels keep a copy in LDS.  The tables
// of a class or pair tag set travel beside it: Tags::tc on the host, a device copy behind
// KParams::cls in the kernels.)
struct TagSet {
  int n;                                   // distinct lowercase tags
  int len[kMaxTags];
  uint8_t name[kMaxTags][kMaxTagLen + 1];  // lowercase ASCII (class tags: see TagClasses)
};

QMX_HD uint8_t lower_ascii(uint8_t c) { return (c >= 'A' && c <= 'Z') ? (uint8_t)(c + 32) : c; }
QMX_HD int utf8_lead_len(uint8_t c) { return c >= 0xF0 ? 4 : c >= 0xE0 ? 3 : c >= 0xC0 ? 2 : 1; }

// Pattern byte i of pattern `pat` (pat < n: open "<t>", pat >= n: close "</t>").
QMX_HD int pattern_len(const TagSet& ts, int pat) {
  return pat < ts.n ? ts.len[pat] + 2 : ts.len[pat - ts.n] + 3;
}
QMX_HD uint8_t pattern_byte(const TagSet& ts, int pat, int i) {
  bool close = pat >= ts.n;
  int t = close ? pat - ts.n : pat;
  if (i == 0) return '<';
  if (close) {
    if (i == 1) return '/';
    --i;
  }
  return i <= ts.len[t] ? ts.name[t][i - 1] : (uint8_t)'>';
}

// Token at position p of x[0:n): +(t+1) open tag t, -(t+1) close tag t, 0 none.
template <class R>
QMX_HD int match_at(const R& x, int n, int p, const TagSet& ts, int* tok_len) {
  if (x[p] != '<') return 0;
  bool close = (p + 1 < n && x[p + 1] == '/');
  int s = p + 1 + (close ? 1 : 0);
  for (int t = 0; t < ts.n; ++t) {
    int L = ts.len[t];
    if (s + L >= n) continue;  // need x[s+L] == '>'
    bool ok = x[s + L] == '>';
    for (int i = 0; ok && i < L; ++i) ok = lower_ascii(x[s + i]) == ts.name[t][i];
    if (ok) {
      *tok_len = s + L + 1 - p;
      return close ? -(t + 1) : (t + 1);
    }
  }
  return 0;
}

// Is x[q:n) (lowercased) a prefix of some pattern?  opens_only: open patterns only.
template <class R>
QMX_HD bool pattern_prefix(const R& x, int q, int n, const TagSet& ts, bool opens_only) {
  int m = n - q;
  int npat = opens_only ? ts.n : 2 * ts.n;
  for (int pat = 0; pat < npat; ++pat) {
    int P = pattern_len(ts, pat);
    if (m > P) continue;
    bool ok = true;
    for (int i = 0; ok && i < m; ++i) ok = lower_ascii(x[q + i]) == pattern_byte(ts, pat, i);
    if (ok) return true;
  }
  return false;
}

// ---------------------------------------------------------------------------
// class tags: one code point per element (TAGS_CLASS; tc: the set's TagClasses)
// ---------------------------------------------------------------------------
// Does class element `k` accept the ASCII byte c?  The streaming filter's regex has no DOTALL
// (a dot rejects '\n' there); the final strip's has.
QMX_HD bool class_accepts(const TagClasses& tc, int k, uint8_t c, bool strip) {
  if (c == '\n' && (tc.flags[k] & CLS_DOT)) return strip;
  return (tc.tab[k][c >> 5] >> (c & 31)) & 1u;
}

// The character at x[s] (a byte >= 0x80, `ln` bytes by its lead byte) at a position of a class with
// a shorthand.  1: accepted, 0: not, -1: cut short at n (a proper prefix, whatever it would have been),
// kWalkHost: a class with a shorthand on the device — the tables of \d, \w and \s are host
// data (qmx_unicode_classes.h), so the host decides.
constexpr int kWalkHost = -2;
inline bool shorthand_holds(uint8_t flags, uint32_t cp) {  // (a host function: the tables are host data)
  auto in = [cp](const uint32_t (*r)[2], int n) {
    int lo = 0, hi = n;  // first range whose last member is >= cp
    while (lo < hi) {
      const int m = (lo + hi) >> 1;
      if (r[m][1] < cp) lo = m + 1;
      else hi = m;
    }
    return lo < n && r[lo][0] <= cp;
  };
  return ((flags & CLS_SH_DIGIT) && in(kDigitRanges, kDigitRangeCount)) ||
         ((flags & CLS_SH_WORD) && in(kWordRanges, kWordRangeCount)) ||
         ((flags & CLS_SH_SPACE) && in(kSpaceRanges, kSpaceRangeCount));
}
template <class R>
QMX_HD int shorthand_char_at(const R& x, int n, int s, uint8_t f, int ln) {  // f: the class's flags, a shorthand bit among them
#ifdef __HIP_DEVICE_COMPILE__
  return kWalkHost;
#else
  if (s + ln > n) return -1;
  uint32_t cp = 0xFFFFFFFFu;  // (a stray continuation byte: no member)
  if (ln == 2) cp = ((x[s] & 0x1Fu) << 6) | (x[s + 1] & 0x3Fu);
  else if (ln == 3) cp = ((x[s] & 0x0Fu) << 12) | ((x[s + 1] & 0x3Fu) << 6) | (x[s + 2] & 0x3Fu);
  else if (ln == 4) cp = ((x[s] & 0x07u) << 18) | ((x[s + 1] & 0x3Fu) << 12) | ((x[s + 2] & 0x3Fu) << 6) | (x[s + 3] & 0x3Fu);
  return shorthand_holds(f, cp) != ((f & CLS_WIDE) != 0) ? 1 : 0;
#endif
}

// Open-ended positions (TagClasses::rep).  Does the repeated class k accept the byte c as one more
// copy, as far as a byte tells: its ASCII table, or a byte >= 0x80 where the class holds any (wide,
// or a shorthand — which code points, only the host knows)?
QMX_HD bool repeat_accepts(const TagClasses& tc, int k, uint8_t c, bool strip) {
  return c < 0x80 ? class_accepts(tc, k, c, strip) : (tc.flags[k] & (CLS_WIDE | CLS_SH)) != 0;
}
// How a walk treats the text after the last copy of an open-ended position.
//   WALK_EXACT: the host walks take the whole run, whatever its characters;
//   WALK_ROWS:  the device walks of a set without kVarRuns never do (kWalkHost), so the byte lengths
//               they see are the rows', bounded by make_tags;
//   WALK_RUNS:  the device walks of a set with kVarRuns take a run of ASCII copies with a cursor of
//               their own and leave to the host (kWalkHost, a suspect candidate) only what a byte
//               cannot tell: a byte >= 0x80 where the class holds any, an accepted '<' or '>'.
// The rule is a template argument, not a matter of which compiler runs: the host compiles WALK_RUNS
// too (bindings.cpp class_candidates, tools/csrc/fuzz_host.cpp) and wherever it answers it answers as
// WALK_EXACT does.
enum : int { WALK_EXACT = 0, WALK_ROWS = 1, WALK_RUNS = 2 };
#ifdef __HIP_DEVICE_COMPILE__
constexpr int kWalkRule = WALK_ROWS;
#else
constexpr int kWalkRule = WALK_EXACT;
#endif
// The run of WALK_RUNS (arguments and answers: repeat_run): ASCII copies other than '<' and '>' are
// taken; kWalkHost at a byte >= 0x80 the class may hold and at a '<' or '>' it accepts (a class may
// swallow the next tag's start: token starts are no longer fixed).  In line in the candidate walks,
// which are out of line themselves (qmx_hip.hip runs_cand_dev, mixed_runs_cand_dev).
template <class R>
QMX_HD int ascii_run(const R& x, int n, int* s, int s0, const TagClasses& tc, int k, bool strip) {
  const uint8_t f = tc.flags[k];
  int q = *s;
  while (true) {
    if (q >= n) return -1;
    const uint8_t c = x[q];
    if (c >= 0x80) {
      if (f & (CLS_WIDE | CLS_SH)) return kWalkHost;
      break;
    }
    if (!class_accepts(tc, k, c, strip)) break;
    if (c == '<' || c == '>') return kWalkHost;
    if (q + 1 - s0 > kMaxTagLen) return 0;
    ++q;
  }
  *s = q;
  return 1;
}
// The run after the copies of an open-ended position of class k, *s the index after the last copy
// and s0 where the tag's name starts.  Host: consumes while the class accepts the next character
// (the element's own logic: ASCII table, wide, shorthand ranges).  1: the run ended before a
// character it does not accept (*s after the run);  -1: the text ended inside the run, or inside
// a character of it;  0: the name would pass kMaxTagLen bytes — "</" + match + ">" is at most
// kMaxTail, the holdback's size — which is no match.  WALK_ROWS: 1 where the next byte is not
// accepted (or the text ended: the caller's proper prefix), kWalkHost where it is.  WALK_RUNS:
// ascii_run, the host's answers over ASCII copies.
// (Out of line, as the mixed walks are: the class kernels keep their register budget —
// tests/test_isa_class_grid.py — and only a set with an open-ended row comes here.)
template <int W = kWalkRule, class R>
__attribute__((noinline)) QMX_HD int repeat_run(const R& x, int n, int* s, int s0, const TagClasses& tc, int k, bool strip) {
  if constexpr (W == WALK_ROWS) {
    return *s < n && repeat_accepts(tc, k, x[*s], strip) ? kWalkHost : 1;
  } else if constexpr (W == WALK_RUNS) {
    return ascii_run(x, n, s, s0, tc, k, strip);
  } else {
    const uint8_t f = tc.flags[k];
    int q = *s;
    while (true) {
      if (q >= n) return -1;
      const uint8_t c = x[q];
      int ln = 1;
      if (c < 0x80) {
        if (!class_accepts(tc, k, c, strip)) break;
      } else {
        if (!(f & (CLS_WIDE | CLS_SH))) break;
        ln = utf8_lead_len(c);
        if (q + ln - s0 > kMaxTagLen) return 0;  // (no follower of such a class takes a byte >= 0x80: no match either way)
        if (f & CLS_SH) {
          const int r = shorthand_char_at(x, n, q, f, ln);
          if (r == 0) break;
          if (r != 1) return r;
        }
        if (q + ln > n) return -1;
      }
      if (q + ln - s0 > kMaxTagLen) return 0;
      q += ln;
    }
    *s = q;
    return 1;
  }
}

// Walk pattern `pat` (pat < n: "<t>", else "</t>") over x[p:n).  1: it matches, *end is the
// index after its '>';  0: mismatch;  -1: every byte of x[p:n) matched and the text ended
// before the pattern did (a proper prefix — a code point cut short at n counts as one);
// kWalkHost: device code met a byte >= 0x80 at a class with a shorthand (shorthand_char_at), or one
// more copy after an open-ended position (repeat_run).
template <int W = kWalkRule, class R>
QMX_HD int class_walk(const R& x, int n, int p, const TagSet& ts, const TagClasses& tc, int pat, bool strip,
                      int* end) {
  const bool close = pat >= ts.n;
  const int t = close ? pat - ts.n : pat;
  int s = p;
  if (s >= n) return -1;
  if (x[s] != '<') return 0;
  ++s;
  if (close) {
    if (s >= n) return -1;
    if (x[s] != '/') return 0;
    ++s;
  }
  constexpr bool kWalkRuns = W != WALK_ROWS;
  const int s0 = s;     // the name starts here; opened: a run was taken, so its length is no longer the row's
  bool opened = false;
  for (int i = 0; i < ts.len[t]; ++i) {
    if (kWalkRuns && opened && s - s0 >= kMaxTagLen) return 0;
    if (s >= n) return -1;
    const uint8_t c = x[s], e = ts.name[t][i];
    if (e < 0x80) {
      if (lower_ascii(c) != e) return 0;
      ++s;
      continue;
    }
    if (c < 0x80) {
      if (!class_accepts(tc, e - 0x80, c, strip)) return 0;
      ++s;
    } else {
      const uint8_t f = tc.flags[e - 0x80];
      if (!(f & (CLS_WIDE | CLS_SH))) return 0;
      const int ln = c >= 0xF0 ? 4 : c >= 0xE0 ? 3 : c >= 0xC0 ? 2 : 1;
      if (kWalkRuns && opened && s + ln - s0 > kMaxTagLen) return 0;
      if (f & CLS_SH) {
        if constexpr (W != WALK_EXACT) {
          return kWalkHost;  // (the tables of \d, \w and \s are host data)
        } else {
          const int r = shorthand_char_at(x, n, s, f, ln);
          if (r != 1) return r;
        }
      }
      if (s + ln > n) return -1;
      s += ln;
    }
    if (__builtin_expect((tc.rep[t] >> i) & 1, 0)) {
      const int r = repeat_run<W>(x, n, &s, s0, tc, e - 0x80, strip);
      if (r != 1) return r;
      opened = true;
    }
  }
  if (s >= n) return -1;
  if (x[s] != '>') return 0;
  *end = s + 1;
  return 1;
}

// match_at for a class tag set: the open of every tag in list order, then (x[p+1] == '/':
// the first element of a tag is a literal, never '/') the close of every tag.
template <class R>
QMX_HD int class_match_at(const R& x, int n, int p, const TagSet& ts, const TagClasses& tc, bool strip,
                          int* tok_len) {
  if (x[p] != '<') return 0;
  const bool close = (p + 1 < n && x[p + 1] == '/');
  for (int t = 0; t < ts.n; ++t) {
    int end = 0;
    if (class_walk(x, n, p, ts, tc, close ? ts.n + t : t, strip, &end) == 1) {
      *tok_len = end - p;
      return close ? -(t + 1) : (t + 1);
    }
  }
  return 0;
}

// The suspect rule of the GPU kernels, which keep their token model (one pattern per '<',
// fixed byte length, no overlapping tokens) by deciding only unambiguous windows: the
// candidate '<' at p against the open (x[p+1] == '/': the close) of every tag that has a class
// element, pattern positions in order.  A literal mismatch or a byte outside a class's table
// rejects that tag; a '<', '>' or non-ASCII byte AT a class position makes the candidate
// suspect — a class may swallow it, so token lengths and starts are no longer fixed, and the
// exact host path decides the stream.  CC_MATCH: the first tag in list order that matches,
// every class position one ASCII byte (*tok, *tok_len as match_at).  Text that ends before a
// pattern does is no match here (the holdback's prefix tests look at it).
// A set with a variable-width tag (TagClasses::var): such a byte at a class position is a plain
// mismatch of that row where the exact walk returns 0 — a '<' or '>' the class's table does not
// accept, a byte >= 0x80 at a class that is not CLS_WIDE.  The rows of `t[0-9]?` are `t[0-9]`
// and `t`: the '>' of every plain "<t>" lies on the class position of the first.  A byte the
// class accepts stays suspect.
enum : int { CC_NONE = 0, CC_MATCH = 1, CC_SUSPECT = 2 };
// c: '<', '>' or >= 0x80 at a position of class k — a mismatch (not a suspect) of the row?
// (A class with a shorthand holds some code points >= 0x80 — which, only the host knows: suspect.)
QMX_HD bool variant_mismatch(const TagClasses& tc, int k, uint8_t c) {
  if ((tc.var & kVarRows) == 0) return false;
  return c >= 0x80 ? !(tc.flags[k] & (CLS_WIDE | CLS_SH)) : !((tc.tab[k][c >> 5] >> (c & 31)) & 1u);
}
// An open-ended position (TagClasses::rep) of row t has matched its last copy and the byte after it,
// x[q], where the follower or the '>' should stand, is one the repeated class accepts: the run is
// longer than the row, so the token's length is not the row's — suspect, the host's exact walk decides.
// (Out of line as repeat_run is, the test of the bit too: in line, even that one load takes the
// class grid kernel past its 256 VGPRs — profiles/repeat_tags/NOTES.md.)
template <class R>
__attribute__((noinline)) QMX_HD bool repeat_suspect(const R& x, int n, int q, const TagClasses& tc, int t, int i, int k,
                                                     bool strip) {
  if (((tc.rep[t] >> i) & 1) == 0) return false;
  return q < n && repeat_accepts(tc, k, x[q], strip);
}
// The run of a candidate walk (RUNS: a set with kVarRuns, the rule of WALK_RUNS): position i of row
// t, of class k, has matched at x[*s - 1].  Where it is open-ended the cursor moves over the ASCII
// copies that follow.  CC_NONE: go on at *s (no open-ended position, or the run ended before a byte
// the class does not accept);  CC_SUSPECT: a byte >= 0x80 the class may hold, or a '<' or '>' it
// accepts;  CC_MATCH — read as "mismatch of the row" —: the text ended inside the run, or the name
// would pass kMaxTagLen bytes.
template <class R>
QMX_HD int candidate_run(const R& x, int n, int* s, int s0, const TagClasses& tc, int t, int i, int k, bool strip) {
  if (((tc.rep[t] >> i) & 1) == 0) return CC_NONE;
  const int r = ascii_run(x, n, s, s0, tc, k, strip);
  return r == 1 ? CC_NONE : r == kWalkHost ? CC_SUSPECT : CC_MATCH;
}
// RUNS: the walk has a cursor of its own, s, which a run moves past the row's position (s0 + i
// without one); a match's length is the row's plus the extra copies of all its runs.
template <bool RUNS = false, class R>
QMX_HD int class_candidate(const R& x, int n, int p, const TagSet& ts, const TagClasses& tc, bool strip, int* tok,
                           int* tok_len) {
  const bool close = p + 1 < n && x[p + 1] == '/';
  const int s0 = p + (close ? 2 : 1);
  int res = CC_NONE;
  for (int t = 0; t < ts.n; ++t) {
    const int L = ts.len[t];
    bool has = false;
      for (int i = 0; i < L; ++i) has = has || ts.name[t][i] >= 0x80;
    if (!has) continue;
    bool ok = true;
    int s = s0;  // (RUNS only: the text position of row position i)
      for (int i = 0; ok && i < L; ++i) {
      if constexpr (!RUNS) s = s0 + i;
      if (s >= n || (RUNS && s - s0 >= kMaxTagLen)) {
        ok = false;
        break;
      }
      const uint8_t c = x[s], e = ts.name[t][i];
      if (e < 0x80) ok = lower_ascii(c) == e;
      else if (c == '<' || c == '>' || c >= 0x80) {
        if (!variant_mismatch(tc, e - 0x80, c)) return CC_SUSPECT;
        ok = false;
      } else {
        ok = class_accepts(tc, e - 0x80, c, strip);
        if constexpr (RUNS) {
          if (ok) {
            ++s;
            const int r = candidate_run(x, n, &s, s0, tc, t, i, e - 0x80, strip);
            if (r == CC_SUSPECT) return CC_SUSPECT;
            ok = r == CC_NONE;
            continue;
          }
        } else {
          if (ok && repeat_suspect(x, n, s0 + i + 1, tc, t, i, e - 0x80, strip)) return CC_SUSPECT;
        }
      }
      if constexpr (RUNS) ++s;
    }
    if constexpr (!RUNS) s = s0 + L;
    if (ok && res == CC_NONE && s < n && x[s] == '>') {
      res = CC_MATCH;
      *tok = close ? -(t + 1) : (t + 1);
      *tok_len = s + 1 - p;
    }
  }
  return res;
}

// Is x[q:n) a proper class-aware prefix of some open or close pattern (streaming tables)?
// 1: yes, 0: no, kWalkHost: some walk could not tell on the device (never on the host).
template <int W = kWalkRule, class R>
QMX_HD int class_prefix(const R& x, int q, int n, const TagSet& ts, const TagClasses& tc) {
  int res = 0;
  for (int pat = 0; pat < 2 * ts.n; ++pat) {
    int end = 0;
    const int r = class_walk<W>(x, n, q, ts, tc, pat, false, &end);
    if (r == -1) return 1;  // (held: the next tile's candidate meets what a later pattern could not tell)
    if (r == kWalkHost) res = kWalkHost;
  }
  return res;
}

// Is x[q:n), ASCII-lowercased, a prefix of the source text "<" + tag + ">" of some tag?  The
// reference's depth-0 holdback is `startswith` on the source, not a pattern test.
template <class R>
QMX_HD bool source_prefix(const R& x, int q, int n, const TagSet& ts, const TagClasses& tc) {
  const int m = n - q;
  for (int t = 0; t < ts.n; ++t) {
    const int L = tc.srclen[t];
    if (m > L + 2) continue;
    bool ok = true;
      for (int i = 0; ok && i < m; ++i) {
      const uint8_t want = i == 0 ? (uint8_t)'<' : i <= L ? tc.src[t][i - 1] : (uint8_t)'>';
      ok = lower_ascii(x[q + i]) == want;
    }
    if (ok) return true;
  }
  return false;
}

// ---------------------------------------------------------------------------
// pair tags: literal patterns, the text folded on read (TAGS_PAIR)
// ---------------------------------------------------------------------------
// Walk pattern `pat` over x[p:n), every character of the text as the patterns see it: an ASCII
// letter lowercased, the upper member of a pair replaced by its lower member.  Both have the
// same byte length, so the text and the pattern move together.  1: it matches (the token ends
// at p + pattern_len);  0: mismatch;  -1: every byte of x[p:n) matched and the text ended
// before the pattern did (a character cut short at n is a prefix of its folded self).
template <class R>
QMX_HD int fold_walk(const R& x, int n, int p, const TagSet& ts, const TagClasses& tc, int pat) {
  const int P = pattern_len(ts, pat);
  for (int i = 0; i < P;) {
    if (p + i >= n) return -1;
    const uint8_t c = x[p + i];
    if (c < 0xC0) {  // ASCII (a stray continuation byte equals no pattern byte here)
      if (lower_ascii(c) != pattern_byte(ts, pat, i)) return 0;
      ++i;
      continue;
    }
    const int ln = c >= 0xF0 ? 4 : c >= 0xE0 ? 3 : 2;
    if (i + ln > P) return 0;
    const int av = ln < n - (p + i) ? ln : n - (p + i);
    uint32_t have = 0, want = 0;
    for (int k = 0; k < av; ++k) have |= (uint32_t)x[p + i + k] << (8 * k);
    for (int k = 0; k < ln; ++k) want |= (uint32_t)pattern_byte(ts, pat, i + k) << (8 * k);
    const uint32_t m = av >= 4 ? 0xffffffffu : ((1u << (8 * av)) - 1u);
    if (have != (want & m)) {
      bool ok = false;
      for (int f = 0; f < tc.nfold; ++f)
        ok = ok || (tc.fold_len[f] == ln && (tc.fold_up[f] & m) == have && tc.fold_lo[f] == want);
      if (!ok) return 0;
    }
    if (av < ln) return -1;
    i += ln;
  }
  return 1;
}

// match_at for a pair tag set (a folded text matches at most one of the distinct tags)
template <class R>
QMX_HD int fold_match_at(const R& x, int n, int p, const TagSet& ts, const TagClasses& tc, int* tok_len) {
  if (x[p] != '<') return 0;
  const bool close = (p + 1 < n && x[p + 1] == '/');
  for (int t = 0; t < ts.n; ++t) {
    const int pat = close ? ts.n + t : t;
    if (fold_walk(x, n, p, ts, tc, pat) == 1) {
      *tok_len = pattern_len(ts, pat);
      return close ? -(t + 1) : (t + 1);
    }
  }
  return 0;
}

// pattern_prefix for a pair tag set
template <class R>
QMX_HD bool fold_pattern_prefix(const R& x, int q, int n, const TagSet& ts, const TagClasses& tc, bool opens_only) {
  const int npat = opens_only ? ts.n : 2 * ts.n;
  for (int pat = 0; pat < npat; ++pat) {
    if (n - q > pattern_len(ts, pat)) continue;
    if (fold_walk(x, n, q, ts, tc, pat) != 0) return true;
  }
  return false;
}

// ---------------------------------------------------------------------------
// mixed tags: the class rules, the text folded on read (TAGS_MIXED)
// ---------------------------------------------------------------------------
// The character of `ln` bytes packed in `want` (a lowered non-ASCII literal) against the text at
// x[s:n), folded: equal bytes, or the upper member of the pair whose lower member `want` is.
// 1: equal;  0: not;  -1: the text ends inside the character and what is there is a prefix of
// it or of its upper member.  (A mixed tag set's tables: mixed_nfold.)
template <class R>
QMX_HD int fold_char_at(const R& x, int n, int s, uint32_t want, int ln, const TagClasses& tc) {
  const int av = ln < n - s ? ln : n - s;
  uint32_t have = 0;
  for (int k = 0; k < av; ++k) have |= (uint32_t)x[s + k] << (8 * k);
  const uint32_t m = av >= 4 ? 0xffffffffu : ((1u << (8 * av)) - 1u);
  if (have != (want & m)) {
    bool ok = false;
    const int nf = mixed_nfold(tc);
    for (int f = 0; f < nf; ++f)
      ok = ok || (tc.fold_len[f] == ln && (tc.fold_up[f] & m) == have && tc.fold_lo[f] == want);
    if (!ok) return 0;
  }
  return av < ln ? -1 : 1;
}
// class_walk for a mixed tag set: a class position is one the tag's bitmap names, every other
// byte >= 0x80 of name[] starts or continues a literal character, compared with the text folded.
template <int W = kWalkRule, class R>
QMX_HD int mixed_walk(const R& x, int n, int p, const TagSet& ts, const TagClasses& tc, int pat, bool strip,
                      int* end) {
  const bool close = pat >= ts.n;
  const int t = close ? pat - ts.n : pat;
  const uint64_t cm = tc.clsmask[t];
  int s = p;
  if (s >= n) return -1;
  if (x[s] != '<') return 0;
  ++s;
  if (close) {
    if (s >= n) return -1;
    if (x[s] != '/') return 0;
    ++s;
  }
  constexpr bool kWalkRuns = W != WALK_ROWS;
  const int s0 = s;  // (as in class_walk)
  bool opened = false;
  for (int i = 0; i < ts.len[t];) {
    if (kWalkRuns && opened && s - s0 >= kMaxTagLen) return 0;
    if (s >= n) return -1;
    const uint8_t c = x[s], e = ts.name[t][i];
    if ((cm >> i) & 1) {
      const int k = e - 0x80;
      if (c < 0x80) {
        if (!class_accepts(tc, k, c, strip)) return 0;
        ++s;
      } else {
        const uint8_t f = tc.flags[k];
        if (!(f & (CLS_WIDE | CLS_SH))) return 0;
        const int ln = utf8_lead_len(c);
        if (kWalkRuns && opened && s + ln - s0 > kMaxTagLen) return 0;
        if (f & CLS_SH) {
          if constexpr (W != WALK_EXACT) {
            return kWalkHost;
          } else {
            const int r = shorthand_char_at(x, n, s, f, ln);
            if (r != 1) return r;
          }
        }
        if (s + ln > n) return -1;
        s += ln;
      }
      if (__builtin_expect((tc.rep[t] >> i) & 1, 0)) {
        const int r = repeat_run<W>(x, n, &s, s0, tc, k, strip);
        if (r != 1) return r;
        opened = true;
      }
      ++i;
    } else if (e < 0x80) {
      if (lower_ascii(c) != e) return 0;
      ++s;
      ++i;
    } else {
      const int ln = utf8_lead_len(e);
      if (kWalkRuns && opened && s + ln - s0 > kMaxTagLen) return 0;
      uint32_t want = 0;
      for (int k = 0; k < ln; ++k) want |= (uint32_t)ts.name[t][i + k] << (8 * k);
      const int r = fold_char_at(x, n, s, want, ln, tc);
      if (r != 1) return r;
      s += ln;
      i += ln;
    }
  }
  if (s >= n) return -1;
  if (x[s] != '>') return 0;
  *end = s + 1;
  return 1;
}

// match_at for a mixed tag set: list order, as class_match_at
template <class R>
QMX_HD int mixed_match_at(const R& x, int n, int p, const TagSet& ts, const TagClasses& tc, bool strip,
                          int* tok_len) {
  if (x[p] != '<') return 0;
  const bool close = (p + 1 < n && x[p + 1] == '/');
  for (int t = 0; t < ts.n; ++t) {
    int end = 0;
    if (mixed_walk(x, n, p, ts, tc, close ? ts.n + t : t, strip, &end) == 1) {
      *tok_len = end - p;
      return close ? -(t + 1) : (t + 1);
    }
  }
  return 0;
}

// class_candidate for a mixed tag set: the tags the byte matchers cannot decide (TagClasses::walk:
// a class element or a pair character), pattern bytes in order.  An ASCII literal by lowercase
// compare, a non-ASCII literal by its folded bytes (never suspect), a class position by its
// ASCII table; '<', '>' or a byte >= 0x80 AT a class position makes the candidate suspect.  A
// match has the pattern's byte length.
// (RUNS: as class_candidate — a cursor of its own, the match's length the walk's.)
template <bool RUNS = false, class R>
QMX_HD int mixed_candidate(const R& x, int n, int p, const TagSet& ts, const TagClasses& tc, bool strip, int* tok,
                           int* tok_len) {
  const bool close = p + 1 < n && x[p + 1] == '/';
  const int s0 = p + (close ? 2 : 1);
  int res = CC_NONE;
  for (int t = 0; t < ts.n; ++t) {
    if (!((tc.walk >> t) & 1)) continue;
    const int L = ts.len[t];
    const uint64_t cm = tc.clsmask[t];
    bool ok = true;
    int s = s0;  // (RUNS only: the text position of name byte i)
    for (int i = 0; ok && i < L;) {
      if constexpr (!RUNS) s = s0 + i;
      if (s >= n || (RUNS && s - s0 >= kMaxTagLen)) {
        ok = false;
        break;
      }
      const uint8_t c = x[s], e = ts.name[t][i];
      if ((cm >> i) & 1) {
        if (c == '<' || c == '>' || c >= 0x80) {
          if (!variant_mismatch(tc, e - 0x80, c)) return CC_SUSPECT;
          ok = false;
        } else {
          ok = class_accepts(tc, e - 0x80, c, strip);
          if constexpr (RUNS) {
            ++s;
            if (ok) {
              const int r = candidate_run(x, n, &s, s0, tc, t, i, e - 0x80, strip);
              if (r == CC_SUSPECT) return CC_SUSPECT;
              ok = r == CC_NONE;
            }
          } else {
            if (ok && repeat_suspect(x, n, s0 + i + 1, tc, t, i, e - 0x80, strip)) return CC_SUSPECT;
          }
        }
        ++i;
      } else if (e < 0x80) {
        ok = lower_ascii(c) == e;
        ++i;
        if constexpr (RUNS) ++s;
      } else {
        const int ln = utf8_lead_len(e);
        if (RUNS && s + ln - s0 > kMaxTagLen) {
          ok = false;
          break;
        }
        uint32_t want = 0;
        for (int k = 0; k < ln; ++k) want |= (uint32_t)ts.name[t][i + k] << (8 * k);
        ok = fold_char_at(x, n, s, want, ln, tc) == 1;
        i += ln;
        if constexpr (RUNS) s += ln;
      }
    }
    if constexpr (!RUNS) s = s0 + L;
    if (ok && res == CC_NONE && s < n && x[s] == '>') {
      res = CC_MATCH;
      *tok = close ? -(t + 1) : (t + 1);
      *tok_len = s + 1 - p;
    }
  }
  return res;
}

// class_prefix for a mixed tag set
template <int W = kWalkRule, class R>
QMX_HD int mixed_prefix(const R& x, int q, int n, const TagSet& ts, const TagClasses& tc) {
  int res = 0;
  for (int pat = 0; pat < 2 * ts.n; ++pat) {
    int end = 0;
    const int r = mixed_walk<W>(x, n, q, ts, tc, pat, false, &end);
    if (r == -1) return 1;
    if (r == kWalkHost) res = kWalkHost;
  }
  return res;
}

// source_prefix for a mixed tag set: x[q:n), folded, a prefix of "<" + tag source + ">".  A
// byte >= 0x80 of the source starts a literal character (a bracket class has ASCII members).
template <class R>
QMX_HD bool mixed_source_prefix(const R& x, int q, int n, const TagSet& ts, const TagClasses& tc) {
  const int m = n - q;
  for (int t = 0; t < ts.n; ++t) {
    const int L = tc.srclen[t];
    if (m > L + 2) continue;
    bool ok = true;
    for (int i = 0; ok && i < m;) {
      const uint8_t want = i == 0 ? (uint8_t)'<' : i <= L ? tc.src[t][i - 1] : (uint8_t)'>';
      if (want < 0x80) {
        ok = lower_ascii(x[q + i]) == want;
        ++i;
        continue;
      }
      const int ln = utf8_lead_len(want);
      uint32_t w = 0;
      for (int k = 0; k < ln; ++k) w |= (uint32_t)tc.src[t][i - 1 + k] << (8 * k);
      ok = fold_char_at(x, n, q + i, w, ln, tc) != 0;
      i += ln;
    }
    if (ok) return true;
  }
  return false;
}

// ---------------------------------------------------------------------------
// the four families behind one kind
// ---------------------------------------------------------------------------
// Token at position p of x[0:n), as match_at (strip: a class tag set's final-strip tables).
template <class R>
QMX_HD int token_at(TagKind kind, const R& x, int n, int p, const TagSet& ts, const TagClasses& tc, bool strip,
                    int* tok_len) {
  return kind == TAGS_CLASS ? class_match_at(x, n, p, ts, tc, strip, tok_len)
       : kind == TAGS_PAIR  ? fold_match_at(x, n, p, ts, tc, tok_len)
       : kind == TAGS_MIXED ? mixed_match_at(x, n, p, ts, tc, strip, tok_len)
                            : match_at(x, n, p, ts, tok_len);
}

// What the GPU kernels decide at the candidate '<' at p, on the host (qmx_hip.hip class_token and
// fin_class_token): the byte matchers' token for the rows without a class element or a pair
// character, the candidate walk's for the others — with a cursor of its own where the set has
// kVarRuns —, the first of the two in list order.  CC_MATCH (*tok, *tok_len), CC_NONE: no tag here,
// CC_SUSPECT: the kernels hand the stream to the host path.
template <class R>
inline int device_token_at(TagKind kind, const R& x, int n, int p, const TagSet& ts, const TagClasses& tc, bool strip,
                           int* tok, int* tok_len) {
  *tok = 0;
  if (kind == TAGS_PAIR || kind == TAGS_LITERAL) {
    *tok = token_at(kind, x, n, p, ts, tc, strip, tok_len);
    return *tok != 0 ? CC_MATCH : CC_NONE;
  }
  int lit_len = 0, wtok = 0, wlen = 0;
  const int lit = match_at(x, n, p, ts, &lit_len);
  const bool runs = (tc.var & kVarRuns) != 0;
  const int r = kind == TAGS_MIXED ? (runs ? mixed_candidate<true>(x, n, p, ts, tc, strip, &wtok, &wlen)
                                           : mixed_candidate(x, n, p, ts, tc, strip, &wtok, &wlen))
                                   : (runs ? class_candidate<true>(x, n, p, ts, tc, strip, &wtok, &wlen)
                                           : class_candidate(x, n, p, ts, tc, strip, &wtok, &wlen));
  if (r == CC_SUSPECT) return CC_SUSPECT;
  const int a = wtok < 0 ? -wtok : wtok, b = lit < 0 ? -lit : lit;
  if (r == CC_MATCH && (lit == 0 || a < b)) {
    *tok = wtok;
    *tok_len = wlen;
  } else if (lit != 0) {
    *tok = lit;
    *tok_len = lit_len;
  }
  return *tok != 0 ? CC_MATCH : CC_NONE;
}

// Is x[q:n), the text from the last '<', held back at depth `depth`?  A class tag set holds the
// tags' source text outside a block and a proper prefix of a pattern inside one.
template <class R>
QMX_HD bool held_at(TagKind kind, const R& x, int q, int n, const TagSet& ts, const TagClasses& tc, int depth) {
  if (kind == TAGS_CLASS) return depth == 0 ? source_prefix(x, q, n, ts, tc) : class_prefix(x, q, n, ts, tc) == 1;
  if (kind == TAGS_MIXED) return depth == 0 ? mixed_source_prefix(x, q, n, ts, tc) : mixed_prefix(x, q, n, ts, tc) == 1;
  return kind == TAGS_PAIR ? fold_pattern_prefix(x, q, n, ts, tc, depth == 0) : pattern_prefix(x, q, n, ts, depth == 0);
}

// ---------------------------------------------------------------------------
// Unicode (Python str.isspace) whitespace on UTF-8 bytes
// ---------------------------------------------------------------------------
// Byte length of the whitespace char starting at x[p] (0: not whitespace, -1: incomplete).
template <class R>
QMX_HD int ws_at(const R& x, int p, int n) {
  uint8_t c = x[p];
  if (c < 0x80) return (c == ' ' || (c >= 0x09 && c <= 0x0d) || (c >= 0x1c && c <= 0x1f)) ? 1 : 0;
  if (c == 0xC2) {
    if (p + 1 >= n) return -1;
    return (x[p + 1] == 0x85 || x[p + 1] == 0xA0) ? 2 : 0;
  }
  if (c == 0xE1 || c == 0xE2 || c == 0xE3) {
    if (p + 2 >= n) return -1;
    uint8_t b1 = x[p + 1], b2 = x[p + 2];
    if (c == 0xE1) return (b1 == 0x9A && b2 == 0x80) ? 3 : 0;
    if (c == 0xE3) return (b1 == 0x80 && b2 == 0x80) ? 3 : 0;
    if (b1 == 0x80) return ((b2 >= 0x80 && b2 <= 0x8A) || b2 == 0xA8 || b2 == 0xA9 || b2 == 0xAF) ? 3 : 0;
    if (b1 == 0x81) return b2 == 0x9F ? 3 : 0;
    return 0;
  }
  return 0;
}
// Byte length of a whitespace char ENDING at x[e-1] (lo = lower bound), 0 if none.
template <class R>
QMX_HD int ws_before(const R& x, int lo, int e) {
  if (e - 1 >= lo && x[e - 1] < 0x80) return ws_at(x, e - 1, e) == 1 ? 1 : 0;
  if (e - 2 >= lo && ws_at(x, e - 2, e) == 2) return 2;
  if (e - 3 >= lo && ws_at(x, e - 3, e) == 3) return 3;
  return 0;
}
// Python str.strip() on a UTF-8 range.
template <class R>
QMX_HD void ustrip(const R& x, int* a, int* b) {
  while (*a < *b) {
    int w = ws_at(x, *a, *b);
    if (w <= 0) break;
    *a += w;
  }
  while (*b > *a) {
    int w = ws_before(x, *a, *b);
    if (w <= 0) break;
    *b -= w;
  }
}

// Strict UTF-8 validation (Python bytes.decode('utf-8')): no overlongs, no surrogates.
template <class R>
QMX_HD bool utf8_valid(const R& x, int a, int b) {
  int i = a;
  while (i < b) {
    uint8_t c = x[i];
    if (c < 0x80) { ++i; continue; }
    int need;
    uint32_t cp;
    if (c >= 0xC2 && c <= 0xDF) { need = 1; cp = c & 0x1F; }
    else if (c >= 0xE0 && c <= 0xEF) { need = 2; cp = c & 0x0F; }
    else if (c >= 0xF0 && c <= 0xF4) { need = 3; cp = c & 0x07; }
    else return false;
    if (i + need >= b) return false;
    for (int k = 1; k <= need; ++k) {
      uint8_t d = x[i + k];
      if ((d & 0xC0) != 0x80) return false;
      cp = (cp << 6) | (d & 0x3F);
    }
    if (need == 2 && (cp < 0x800 || (cp >= 0xD800 && cp <= 0xDFFF))) return false;
    if (need == 3 && (cp < 0x10000 || cp > 0x10FFFF)) return false;
    i += need + 1;
  }
  return true;
}

// Decode one (W)UTF-8 code point at y[p] (input known well-formed WTF-8); returns length.
template <class R>
QMX_HD int wtf8_decode(const R& y, int p, int n, uint32_t* cp) {
  uint8_t c = y[p];
  if (c < 0x80) { *cp = c; return 1; }
  if (c < 0xE0 && p + 1 < n) { *cp = ((c & 0x1F) << 6) | (y[p + 1] & 0x3F); return 2; }
  if (c < 0xF0 && p + 2 < n) {
    *cp = ((c & 0x0F) << 12) | ((y[p + 1] & 0x3F) << 6) | (y[p + 2] & 0x3F);
    return 3;
  }
  if (p + 3 < n) {
    *cp = ((c & 0x07) << 18) | ((y[p + 1] & 0x3F) << 12) | ((y[p + 2] & 0x3F) << 6) | (y[p + 3] & 0x3F);
    return 4;
  }
  *cp = 0xFFFD;
  return 1;
}

QMX_HD bool is_cont(uint8_t c) { return (c & 0xC0) == 0x80; }

// ---------------------------------------------------------------------------
// JSON string escaping, json.dumps(ensure_ascii=True) byte-exact
// ---------------------------------------------------------------------------
QMX_HD int escaped_len_cp(uint32_t cp) {
  if (cp >= 0x20 && cp < 0x7F && cp != '"' && cp != '\\') return 1;  // common case first
  if (cp == '"' || cp == '\\' || cp == '\n' || cp == '\r' || cp == '\t' || cp == 0x08 || cp == 0x0C) return 2;
  if (cp >= 0x20 && cp <= 0x7E) return 1;
  if (cp < 0x10000) return 6;
  return 12;
}
QMX_HD uint8_t hexd(uint32_t v) { return (uint8_t)(v < 10 ? '0' + v : 'a' + v - 10); }
QMX_HD int write_u4(uint8_t* o, uint32_t u) {
  o[0] = '\\'; o[1] = 'u';
  o[2] = hexd((u >> 12) & 15); o[3] = hexd((u >> 8) & 15); o[4] = hexd((u >> 4) & 15); o[5] = hexd(u & 15);
  return 6;
}
QMX_HD int escape_cp(uint32_t cp, uint8_t* o) {
  if (cp >= 0x20 && cp < 0x7F && cp != '"' && cp != '\\') {  // common case first (no switch tree)
    o[0] = (uint8_t)cp;
    return 1;
  }
  switch (cp) {
    case '"': o[0] = '\\'; o[1] = '"'; return 2;
    case '\\': o[0] = '\\'; o[1] = '\\'; return 2;
    case '\n': o[0] = '\\'; o[1] = 'n'; return 2;
    case '\r': o[0] = '\\'; o[1] = 'r'; return 2;
    case '\t': o[0] = '\\'; o[1] = 't'; return 2;
    case 0x08: o[0] = '\\'; o[1] = 'b'; return 2;
    case 0x0C: o[0] = '\\'; o[1] = 'f'; return 2;
    default: break;
  }
  if (cp >= 0x20 && cp <= 0x7E) { o[0] = (uint8_t)cp; return 1; }
  if (cp < 0x10000) return write_u4(o, cp);
  uint32_t v = cp - 0x10000;
  write_u4(o, 0xD800 | (v >> 10));
  write_u4(o + 6, 0xDC00 | (v & 0x3FF));
  return 12;
}

// ---------------------------------------------------------------------------
// JSON string decode (into WTF-8) — the body between the quotes, already validated
// ---------------------------------------------------------------------------
QMX_HD int hexv(uint8_t c) {
  if (c >= '0' && c <= '9') return c - '0';
  c = lower_ascii(c);
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  return -1;
}
template <class R>
QMX_HD uint32_t hex4(const R& x, int i) {
  return (uint32_t)((hexv(x[i]) << 12) | (hexv(x[i + 1]) << 8) | (hexv(x[i + 2]) << 4) | hexv(x[i + 3]));
}
QMX_HD int put_wtf8(uint32_t cp, uint8_t* o) {
  if (cp < 0x80) { if (o) o[0] = (uint8_t)cp; return 1; }
  if (cp < 0x800) { if (o) { o[0] = 0xC0 | (cp >> 6); o[1] = 0x80 | (cp & 0x3F); } return 2; }
  if (cp < 0x10000) {
    if (o) { o[0] = 0xE0 | (cp >> 12); o[1] = 0x80 | ((cp >> 6) & 0x3F); o[2] = 0x80 | (cp & 0x3F); }
    return 3;
  }
  if (o) {
    o[0] = 0xF0 | (cp >> 18); o[1] = 0x80 | ((cp >> 12) & 0x3F);
    o[2] = 0x80 | ((cp >> 6) & 0x3F); o[3] = 0x80 | (cp & 0x3F);
  }
  return 4;
}
// Decode JSON string body x[a:b) → out (may be null: length only). Python json semantics:
// \uD8xx\uDCxx pairs combine, lone surrogates are kept (as 3-byte WTF-8).
template <class R>
QMX_HD int json_unescape(const R& x, int a, int b, uint8_t* out) {
  int o = 0, i = a;
  while (i < b) {
    uint8_t c = x[i];
    if (c != '\\') {
      if (out) out[o] = c;
      ++o; ++i;
      continue;
    }
    uint8_t e = x[i + 1];
    uint32_t cp;
    if (e == 'u') {
      cp = hex4(x, i + 2);
      i += 6;
      if (cp >= 0xD800 && cp <= 0xDBFF && i + 6 <= b && x[i] == '\\' && x[i + 1] == 'u') {
        uint32_t lo = hex4(x, i + 2);
        if (lo >= 0xDC00 && lo <= 0xDFFF) {
          cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
          i += 6;
        }
      }
    } else {
      i += 2;
      switch (e) {
        case 'n': cp = '\n'; break;
        case 't': cp = '\t'; break;
        case 'r': cp = '\r'; break;
        case 'b': cp = 0x08; break;
        case 'f': cp = 0x0C; break;
        default: cp = e; break;  // " \ /
      }
    }
    o += put_wtf8(cp, out ? out + o : nullptr);
  }
  return o;
}

// ---------------------------------------------------------------------------
// Validating JSON delta extractor (Python json.loads + quorum's exception semantics)
// ---------------------------------------------------------------------------
// Literals are packed into 64-bit immediates (byte k = char k): device code must never
// index string literals in per-byte loops (that is a global-memory load per byte).
constexpr uint64_t pack_lit(const char* s) {
  uint64_t v = 0;
  for (int k = 0; s[k] && k < 8; ++k) v |= (uint64_t)(uint8_t)s[k] << (8 * k);
  return v;
}
constexpr int lit_len(const char* s) {
  int k = 0;
  while (s[k]) ++k;
  return k;
}
// packed with the LAST char in the lowest byte (for a left-shifting rolling window)
constexpr uint64_t pack_rev(const char* s) {
  uint64_t v = 0;
  int n = lit_len(s);
  for (int k = 0; k < n; ++k) v = (v << 8) | (uint8_t)s[k];
  return v;
}
QMX_HD uint8_t lit_ch(uint64_t v, int k) { return (uint8_t)(v >> (8 * k)); }

enum EvKind : int { EV_SKIP = 0, EV_CONTENT = 1, EV_ABORT = 2 };
struct EvResult {
  int kind;
  int str_a, str_b;  // content string body (between quotes) when kind == EV_CONTENT
};

enum : int { K_NONE = 0, K_OBJ, K_ARR, K_STR, K_NUM, K_TRUE, K_FALSE, K_NULL };
enum : int { R_NONE = 0, R_ROOT, R_CHOICES, R_C0, R_DELTA, R_CONTENT, R_ROOTELEM, R_DELTAELEM };

// small KMP-free matcher for the two substring targets (no self-overlap issues handled
// generically: we restart at each code unit with a tiny window compare)
struct StrScan {
  bool ok;
  bool eq_choices, eq_delta, eq_content;
  bool has_choices, has_content;
  bool nonempty;
  int end;  // position after closing quote
};

// Scan a JSON string starting at x[p] == '"'.  Validates (control chars, escapes) and
// computes equality / containment against the fixed ASCII targets on DECODED chars.
template <class R>
QMX_HD StrScan scan_string(const R& x, int p, int b, bool want_contains) {
  StrScan r;
  r.ok = false; r.eq_choices = r.eq_delta = r.eq_content = false;
  r.has_choices = r.has_content = false; r.nonempty = false; r.end = p;
  constexpr uint64_t T0 = pack_lit("choices"), T1 = pack_lit("delta"), T2 = pack_lit("content");
  constexpr uint64_t R0 = pack_rev("choices"), R2 = pack_rev("content");
  constexpr uint64_t M56 = (1ull << 56) - 1;
  int k = 0;               // decoded unit index
  bool e0 = true, e1 = true, e2 = true;
  // rolling window of the last 7 decoded units (ASCII, 0 for non-ASCII), newest in byte 0
  uint64_t win = 0;
  int i = p + 1;
  while (true) {
    if (i >= b) return r;
    uint8_t c = x[i];
    uint32_t u;  // decoded unit: ASCII char or 0x100 for "other"
    if (c == '"') { ++i; break; }
    if (c < 0x20) return r;
    if (c == '\\') {
      if (i + 1 >= b) return r;
      uint8_t e = x[i + 1];
      if (e == 'u') {
        if (i + 5 >= b) return r;
        for (int q = 2; q < 6; ++q) if (hexv(x[i + q]) < 0) return r;
        uint32_t cp = hex4(x, i + 2);
        u = cp < 0x80 ? cp : 0x100;
        i += 6;
      } else {
        switch (e) {
          case '"': u = '"'; break;
          case '\\': u = '\\'; break;
          case '/': u = '/'; break;
          case 'b': u = 0x08; break;
          case 'f': u = 0x0C; break;
          case 'n': u = '\n'; break;
          case 'r': u = '\r'; break;
          case 't': u = '\t'; break;
          default: return r;
        }
        i += 2;
      }
    } else if (c >= 0x80) {
      // one code point = one "other" unit; skip its continuation bytes
      int ln = c >= 0xF0 ? 4 : c >= 0xE0 ? 3 : 2;
      u = 0x100;
      i += ln;
    } else {
      u = c;
      ++i;
    }
    e0 = e0 && k < 7 && u == lit_ch(T0, k);
    e1 = e1 && k < 5 && u == lit_ch(T1, k);
    e2 = e2 && k < 7 && u == lit_ch(T2, k);
    ++k;
    if (want_contains) {
      win = ((win << 8) | (u < 0x80 ? u : 0u)) & M56;
      r.has_choices = r.has_choices || (k >= 7 && win == R0);
      r.has_content = r.has_content || (k >= 7 && win == R2);
    }
  }
  r.ok = true;
  r.eq_choices = e0 && k == 7;
  r.eq_delta = e1 && k == 5;
  r.eq_content = e2 && k == 7;
  r.nonempty = k > 0;
  r.end = i;
  return r;
}

struct NumScan {
  bool ok;
  bool zero;
  int end;
};
// Python NUMBER_RE: -?(0|[1-9]\d*)(\.\d+)?([eE][-+]?\d+)?  (+ float underflow to 0.0)
template <class R>
QMX_HD NumScan scan_number(const R& x, int p, int b) {
  NumScan r{false, true, p};
  int i = p;
  if (i < b && x[i] == '-') ++i;
  if (i >= b) return r;
  int first_nz_exp = 0;  // decimal exponent of first nonzero digit (before applying e)
  bool seen_nz = false;
  int int_start = i;
  if (x[i] == '0') {
    ++i;
  } else if (x[i] >= '1' && x[i] <= '9') {
    while (i < b && x[i] >= '0' && x[i] <= '9') ++i;
  } else {
    return r;
  }
  int int_len = i - int_start;
  for (int q = int_start; q < i; ++q)
    if (x[q] != '0') { seen_nz = true; first_nz_exp = int_len - 1 - (q - int_start); break; }
  bool is_float = false;
  if (i + 1 < b && x[i] == '.' && x[i + 1] >= '0' && x[i + 1] <= '9') {
    is_float = true;
    ++i;
    int f0 = i;
    while (i < b && x[i] >= '0' && x[i] <= '9') {
      if (!seen_nz && x[i] != '0') { seen_nz = true; first_nz_exp = -(i - f0 + 1); }
      ++i;
    }
  }
  if (i < b && (x[i] == 'e' || x[i] == 'E')) {
    int j = i + 1;
    bool neg = false;
    if (j < b && (x[j] == '+' || x[j] == '-')) { neg = x[j] == '-'; ++j; }
    if (j < b && x[j] >= '0' && x[j] <= '9') {
      is_float = true;
      long ev = 0;
      while (j < b && x[j] >= '0' && x[j] <= '9') {
        if (ev < 100000) ev = ev * 10 + (x[j] - '0');
        ++j;
      }
      i = j;
      if (seen_nz && is_float) {
        long e10 = first_nz_exp + (neg ? -ev : ev);
        if (e10 < -324) seen_nz = false;  // underflows to 0.0
      }
    }
  }
  r.ok = true;
  r.zero = !seen_nz;
  r.end = i;
  return r;
}

template <class R>
QMX_HD bool lit_at(const R& x, int p, int b, uint64_t lit, int len) {
  if (p + len > b) return false;
  for (int i = 0; i < len; ++i)
    if (x[p + i] != lit_ch(lit, i)) return false;
  return true;
}
#define QMX_LIT(s) pack_lit(s), lit_len(s)

QMX_HD bool json_ws(uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

// Classify one framed SSE event e[0:m) (see reference.classify_event for the contract).
template <class R>
QMX_HD EvResult classify_event(const R& e, int m) {
  EvResult res{EV_SKIP, 0, 0};
  if (!lit_at(e, 0, m, QMX_LIT("data: "))) return res;
  if (!utf8_valid(e, 0, m)) return res;
  int a = 6, b = m;
  ustrip(e, &a, &b);
  if (b - a == 6 && lit_at(e, a, b, QMX_LIT("[DONE]"))) return res;

  // --- parse ---------------------------------------------------------------------
  uint64_t stk[kJsonMaxDepth / 64] = {0, 0, 0, 0};  // bit = container is array
  int depth = 0;
  int crole[5] = {0, 0, 0, 0, 0};   // role of the container at depth 1..4
  int ccount[5] = {0, 0, 0, 0, 0};  // members/elements seen
  int keyrole = R_NONE;             // role for the next object member value
  // decision state
  int root_kind = K_NONE;
  bool root_has = false;  // root array elem == "choices" / root str contains "choices"
  bool has_choices = false;
  int ch_kind = K_NONE;
  bool ch_truthy = false;
  int c0_kind = K_NONE;
  bool d_present = false;
  int d_kind = K_NONE;
  bool d_has = false;  // delta array elem == "content" / delta str contains "content"
  bool has_content = false;
  int content_kind = K_NONE;
  int ca = 0, cb = 0;

  int pos = a;
  int role = R_ROOT;
  // state: 0 = expect value, 1 = expect key, 2 = after value
  int state = 0;
  int vkind = K_NONE;
  bool vtruthy = false;
  while (true) {
    if (state == 0 || state == 1) {
      while (pos < b && json_ws(e[pos])) ++pos;
      if (pos >= b) return res;  // JSONDecodeError -> skip
    }
    if (state == 1) {
      if (e[pos] != '"') return res;
      StrScan s = scan_string(e, pos, b, false);
      if (!s.ok) return res;
      int cr = depth <= 4 ? crole[depth] : R_NONE;
      keyrole = R_NONE;
      if (cr == R_ROOT && s.eq_choices) {
        keyrole = R_CHOICES;
        has_choices = true; ch_kind = K_NONE; ch_truthy = false; c0_kind = K_NONE;
        d_present = false; d_kind = K_NONE; d_has = false; has_content = false; content_kind = K_NONE;
      } else if (cr == R_C0 && s.eq_delta) {
        keyrole = R_DELTA;
        d_present = true; d_kind = K_NONE; d_has = false; has_content = false; content_kind = K_NONE;
      } else if (cr == R_DELTA && s.eq_content) {
        keyrole = R_CONTENT;
        has_content = true; content_kind = K_NONE;
      }
      pos = s.end;
      while (pos < b && json_ws(e[pos])) ++pos;
      if (pos >= b || e[pos] != ':') return res;
      ++pos;
      role = keyrole;
      state = 0;
      continue;
    }
    if (state == 0) {
      uint8_t c = e[pos];
      if (c == '{' || c == '[') {
        if (depth >= kJsonMaxDepth) { res.kind = EV_ABORT; return res; }
        bool arr = c == '[';
        if (arr) stk[depth >> 6] |= (1ull << (depth & 63));
        else stk[depth >> 6] &= ~(1ull << (depth & 63));
        ++depth;
        if (depth <= 4) { crole[depth] = role; ccount[depth] = 0; }
        if (role == R_ROOT) root_kind = arr ? K_ARR : K_OBJ;
        else if (role == R_CHOICES) ch_kind = arr ? K_ARR : K_OBJ;
        else if (role == R_C0) c0_kind = arr ? K_ARR : K_OBJ;
        else if (role == R_DELTA) d_kind = arr ? K_ARR : K_OBJ;
        else if (role == R_CONTENT) content_kind = arr ? K_ARR : K_OBJ;
        ++pos;
        while (pos < b && json_ws(e[pos])) ++pos;
        if (pos >= b) return res;
        if (e[pos] == (arr ? ']' : '}')) {
          ++pos;
          --depth;
          vkind = arr ? K_ARR : K_OBJ;
          vtruthy = false;
          // role of the just-closed container was `role`
          state = 2;
          goto after_value_container;
        }
        if (arr) {
          // element 0
          int cr = depth <= 4 ? crole[depth] : R_NONE;
          role = cr == R_CHOICES ? R_C0 : cr == R_ROOT ? R_ROOTELEM : cr == R_DELTA ? R_DELTAELEM : R_NONE;
          if (depth <= 4) ccount[depth] = 1;
          state = 0;
        } else {
          if (depth <= 4) ccount[depth] = 1;
          state = 1;
        }
        continue;
      }
      // scalar value
      if (c == '"') {
        bool want = role == R_ROOT || role == R_DELTA;
        StrScan s = scan_string(e, pos, b, want);
        if (!s.ok) return res;
        vkind = K_STR;
        vtruthy = s.nonempty;
        if (role == R_ROOT) root_has = s.has_choices;
        else if (role == R_DELTA) d_has = s.has_content;
        else if (role == R_ROOTELEM) root_has = root_has || s.eq_choices;
        else if (role == R_DELTAELEM) d_has = d_has || s.eq_content;
        else if (role == R_CONTENT) { ca = pos + 1; cb = s.end - 1; }
        pos = s.end;
      } else if (c == '-' || (c >= '0' && c <= '9')) {
        if (c == '-' && lit_at(e, pos, b, pack_lit("-Infinit"), 8) && lit_at(e, pos + 8, b, QMX_LIT("y"))) {
          pos += 9; vkind = K_NUM; vtruthy = true;
        } else {
          NumScan ns = scan_number(e, pos, b);
          if (!ns.ok) return res;
          pos = ns.end; vkind = K_NUM; vtruthy = !ns.zero;
        }
      } else if (lit_at(e, pos, b, QMX_LIT("true"))) { pos += 4; vkind = K_TRUE; vtruthy = true; }
      else if (lit_at(e, pos, b, QMX_LIT("false"))) { pos += 5; vkind = K_FALSE; vtruthy = false; }
      else if (lit_at(e, pos, b, QMX_LIT("null"))) { pos += 4; vkind = K_NULL; vtruthy = false; }
      else if (lit_at(e, pos, b, QMX_LIT("NaN"))) { pos += 3; vkind = K_NUM; vtruthy = true; }
      else if (lit_at(e, pos, b, QMX_LIT("Infinity"))) { pos += 8; vkind = K_NUM; vtruthy = true; }
      else return res;
      if (role == R_ROOT) root_kind = vkind;
      else if (role == R_CHOICES) { ch_kind = vkind; ch_truthy = vtruthy; }
      else if (role == R_C0) c0_kind = vkind;
      else if (role == R_DELTA) d_kind = vkind;
      else if (role == R_CONTENT) content_kind = vkind;
      state = 2;
    }
  after_value_container:
    // state 2: after a complete value at the current depth
    if (state == 2) {
      if (depth == 0) {
        while (pos < b && json_ws(e[pos])) ++pos;
        if (pos != b) return res;  // extra data
        break;
      }
      while (pos < b && json_ws(e[pos])) ++pos;
      if (pos >= b) return res;
      bool arr = (stk[(depth - 1) >> 6] >> ((depth - 1) & 63)) & 1;
      uint8_t c = e[pos];
      if (c == ',') {
        ++pos;
        if (depth <= 4) ++ccount[depth];
        if (arr) {
          role = R_NONE;
          int cr = depth <= 4 ? crole[depth] : R_NONE;
          if (cr == R_ROOT) role = R_ROOTELEM;
          else if (cr == R_DELTA) role = R_DELTAELEM;
          state = 0;
        } else {
          state = 1;
        }
        continue;
      }
      if (c == (arr ? ']' : '}')) {
        ++pos;
        int closed_role = depth <= 4 ? crole[depth] : R_NONE;
        int cnt = depth <= 4 ? ccount[depth] : 1;
        --depth;
        if (closed_role == R_CHOICES) ch_truthy = cnt > 0;
        role = closed_role;
        state = 2;
        goto after_value_container;
      }
      return res;
    }
  }

  // --- quorum decision (oai_proxy.py:608-616 under Python semantics) ---------------
  switch (root_kind) {
    case K_OBJ: break;
    case K_ARR:
    case K_STR: res.kind = root_has ? EV_ABORT : EV_SKIP; return res;
    default: res.kind = EV_ABORT; return res;  // `in` on number/bool/None -> TypeError
  }
  if (!has_choices || !ch_truthy) return res;
  if (ch_kind != K_ARR) { res.kind = EV_ABORT; return res; }
  if (c0_kind != K_OBJ) { res.kind = EV_ABORT; return res; }
  if (!d_present) return res;  // .get("delta", {}) -> {} -> no content
  switch (d_kind) {
    case K_OBJ: break;
    case K_ARR:
    case K_STR: res.kind = d_has ? EV_ABORT : EV_SKIP; return res;
    default: res.kind = EV_ABORT; return res;
  }
  if (!has_content) return res;
  if (content_kind != K_STR) { res.kind = EV_ABORT; return res; }
  res.kind = EV_CONTENT;
  res.str_a = ca;
  res.str_b = cb;
  return res;
}

// Reader adaptors: R is a raw pointer on the host; on the device an LDS word reader.
template <class R>
struct OffsetReader {
  const R& r;
  int off;
  QMX_HD uint8_t operator[](int i) const { return r[off + i]; }
};
// Event at x[e0 : e0+m); string offsets in the result are relative to e0.
template <class R>
QMX_HD EvResult classify_event_at(const R& x, int e0, int m) {
  OffsetReader<R> o{x, e0};
  return classify_event(o, m);
}

}  // namespace qmx
