// qmx_engine.cpp — host engine core + the sequential (oracle-equivalent) CPU algorithms.
#include "qmx_env.h"
#include "qmx_engine.h"
#include "qmx_unicode_fold.h"

#include <cstdlib>
#include <ctime>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <stdexcept>

namespace qmx {

const char* kDeltaSuffix = "\"}, \"finish_reason\": null}]}\n\n";
const char* kFinalSuffix = "\"}, \"finish_reason\": \"stop\"}]}\n\n";

namespace {

// One parsed element of a class tag: a literal byte, or an ASCII acceptance table.
struct Elem {
  bool cls = false;
  uint8_t lit = 0;
  uint32_t tab[4] = {0, 0, 0, 0};
  uint8_t flags = 0;
  bool rep = false;  // the open-ended copy of an unbounded repetition: this element, once or more
  std::string txt;  // as written (a plain literal lowered): tagset_rows
};

bool printable(uint8_t c) { return c >= 0x20 && c < 0x7f; }

// A refusal with a message of its own, thrown inside the tag parsers (build_tags adds the tag).
struct TagRefusal {
  const char* msg;
};
const char* kUpperShorthand =
    "tag holds \\D, \\W or \\S: the reference's streaming filter compiles the lowercased tag (\\d, \\w, \\s) and its "
    "final strip the tag as written, so the two disagree (runs with --impl python): ";
const char* kEmptyRepeat = "tag repeats a group that can match the empty string (runs with --impl python): ";
const char* kUnboundedGroup = "tag repeats a group without a bound (runs with --impl python): ";
const char* kRepeatOverlap =
    "tag repeats an element that also accepts what can follow the run, so the run's end depends on the regex's "
    "backtracking (runs with --impl python): ";

// The shorthand at t[i] == '\\' (make_tags' `extended`): its ASCII table is or-ed into tab and its
// flag bit returned; 0: no shorthand there.  \D, \W and \S are refused with their own message.
uint8_t shorthand_at(const std::string& t, size_t i, uint32_t* tab) {
  if (i + 1 >= t.size()) return 0;
  const char c = t[i + 1];
  if (c == 'D' || c == 'W' || c == 'S') throw TagRefusal{kUpperShorthand};
  const uint32_t* a = c == 'd' ? kDigitAscii : c == 'w' ? kWordAscii : c == 's' ? kSpaceAscii : nullptr;
  if (!a) return 0;
  for (int k = 0; k < 4; ++k) tab[k] |= a[k];
  return c == 'd' ? CLS_SH_DIGIT : c == 'w' ? CLS_SH_WORD : CLS_SH_SPACE;
}

void tab_set(uint32_t* tab, uint8_t c) {  // under IGNORECASE: both cases of a letter
  for (uint8_t v : {c, lower_ascii(c), (uint8_t)((c >= 'a' && c <= 'z') ? c - 32 : c)}) tab[v >> 5] |= 1u << (v & 31);
}

// "[...]" at t[i] == '[': members are printable ASCII literals other than "<>/[", ranges and
// the escapes \\ \] \^ \- \[.  False for everything Python's parser reads differently or
// warns about (a leading ']', "--", "&&", "~~", "||", shorthands, POSIX classes).
// extended: \d, \w and \s are members too (never a range endpoint: an error in re).
bool parse_bracket(const std::string& t, size_t& i, Elem& e, bool extended) {
  size_t j = i + 1;
  bool neg = false;
  if (j < t.size() && t[j] == '^') { neg = true; ++j; }
  if (j < t.size() && t[j] == ']') return false;
  uint32_t tab[4] = {0, 0, 0, 0};
  uint8_t sh = 0;
  // one member byte at t[j] (escapes resolved); '-' is handled by the caller
  auto member = [&](uint8_t* out) {
    if (j >= t.size()) return false;
    uint8_t c = (uint8_t)t[j];
    if (c == '\\') {
      if (j + 1 >= t.size() || !std::strchr("\\]^-[", t[j + 1])) return false;
      *out = (uint8_t)t[j + 1];
      j += 2;
      return true;
    }
    if (!printable(c) || std::strchr("<>/[]", (int)c)) return false;
    *out = c;
    ++j;
    return true;
  };
  const size_t first = j;
  while (true) {
    if (j >= t.size()) return false;  // no closing ']'
    if (t[j] == ']') break;
    if (j + 1 < t.size() && t[j] == t[j + 1] && std::strchr("-&~|", t[j])) return false;
    if (t[j] == '-') {  // a literal only as the first or the last member
      if (j != first && !(j + 1 < t.size() && t[j + 1] == ']')) return false;
      tab_set(tab, '-');
      ++j;
      continue;
    }
    if (extended && t[j] == '\\') {
      const uint8_t f = shorthand_at(t, j, tab);
      if (f) {
        sh |= f;
        j += 2;
        if (j + 1 < t.size() && t[j] == '-' && t[j + 1] != ']') return false;
        continue;
      }
    }
    uint8_t lo;
    if (!member(&lo)) return false;
    if (j + 1 < t.size() && t[j] == '-' && t[j + 1] != ']') {  // range lo-hi
      ++j;
      if (t[j] == '-') return false;
      uint8_t hi;
      if (!member(&hi) || hi < lo) return false;
      for (int c = lo; c <= hi; ++c) tab_set(tab, (uint8_t)c);
    } else {
      tab_set(tab, lo);
    }
  }
  i = j + 1;
  e.cls = true;
  e.flags = (neg ? CLS_WIDE : 0) | sh;
  for (int k = 0; k < 4; ++k) e.tab[k] = neg ? ~tab[k] : tab[k];
  return true;
}

// One element of a class tag at t[i] (a literal, an escape, '.', a bracket class), or false when
// it lies outside the class subset.  wide: a byte >= 0x80 outside a bracket class is a literal
// element of its own (a mixed tag set: the bytes of a non-ASCII literal character, already
// lowered through the pair table).
bool parse_elem(const std::string& t, size_t& i, Elem& e, bool wide, bool extended = false) {
  const uint8_t c = (uint8_t)t[i];
  const size_t i0 = i;
  if (c == '\\' && extended && (e.flags = shorthand_at(t, i, e.tab)) != 0) {
    e.cls = true;  // a shorthand on its own: a class of one member
    i += 2;
  } else if (c == '\\') {
    if (i + 1 >= t.size() || !std::strchr(".^$*+?{}[]\\|()-", t[i + 1])) return false;
    e.lit = (uint8_t)t[i + 1];
    i += 2;
  } else if (c == '.') {
    e.cls = true;
    e.flags = CLS_WIDE | CLS_DOT;
    for (int k = 0; k < 4; ++k) e.tab[k] = ~0u;
    ++i;
  } else if (c == '[') {
    if (!parse_bracket(t, i, e, extended)) return false;
  } else if (wide && c >= 0x80) {
    e.lit = c;
    ++i;
  } else {
    if (!printable(c) || std::strchr("^$*+?{}]|()<>/", (int)c)) return false;
    e.lit = lower_ascii(c);
    ++i;
  }
  e.txt = t.substr(i0, i - i0);
  if (!e.cls && e.txt.size() == 1) e.txt[0] = (char)e.lit;
  return true;
}

// The elements of one tag, or false when it lies outside the class subset.
bool parse_class_tag(const std::string& t, std::vector<Elem>& out, bool wide = false) {
  for (size_t i = 0; i < t.size();) {
    Elem e;
    if (!parse_elem(t, i, e, wide)) return false;
    out.push_back(e);
  }
  return !out.empty() && !out[0].cls;
}

// Variable-width tags (make_tags' `variants`): the class subset plus '?' after an element or a
// group, '|' and groups "(...)" / "(?:...)".  Such a tag has the matches of the ordered
// alternation of its fixed-width expansions, its rows: "x?" is "(?:x|)" (greedy: present
// first), concatenation distributes over ordered alternation and keeps the priority order, and
// a backtracking matcher returns the first success in that order.  A recursive-descent parser
// over alt := seq ('|' seq)*, seq := (atom '?'?)*, atom := element | group.
// With `extended` an element may be a shorthand (\d, \w, \s, alone or in a bracket class) and an
// atom may carry a count instead of the '?': "{m}", "{m,n}" or "{,n}" (VariantParser::counted).
typedef std::vector<Elem> Row;
typedef std::vector<Row> Rows;  // in priority order, no two equal

bool same_elem(const Elem& a, const Elem& b) {
  if (a.cls != b.cls || a.rep != b.rep) return false;
  return a.cls ? a.flags == b.flags && std::memcmp(a.tab, b.tab, sizeof(a.tab)) == 0 : a.lit == b.lit;
}
bool same_row(const Row& a, const Row& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (!same_elem(a[i], b[i])) return false;
  return true;
}

struct TooManyRows {};
struct RowTooLong {};  // a row of more than kMaxTagLen elements: no such row fits "</" + match + ">" in 64 bytes

// l followed by r.  Nested counts multiply the elements of one row ("((a{61}){61}){61}"), so the
// length is bounded here, where a row grows, and not after the expansion.
Row join_rows(const Row& l, const Row& r) {
  if (l.size() + r.size() > (size_t)kMaxTagLen) throw RowTooLong();
  Row c = l;
  c.insert(c.end(), r.begin(), r.end());
  return c;
}

// A later duplicate of a row never matches where the first did not: dropped.  The count of
// distinct rows only grows towards the whole tag, so more than kMaxTags here is more at the end.
void add_row(Rows& rows, const Row& r) {
  for (const Row& have : rows)
    if (same_row(have, r)) return;
  if ((int)rows.size() >= kMaxTags) throw TooManyRows();
  rows.push_back(r);
}

struct VariantParser {
  const std::string& t;
  bool wide;
  bool extended;  // shorthands, and counted repetition after an atom
  bool repeat;    // with extended: '+', '*' and "{m,}" after one element (VariantParser::unbounded)
  size_t i = 0;
  bool ops = false;  // a '?', a '|' or a group was read: a variable-width tag

  bool alt(Rows& out, int depth) {
    do {
      Rows s;
      if (!seq(s, depth)) return false;
      for (const Row& r : s) add_row(out, r);
      if (i >= t.size() || t[i] != '|') return true;
      ops = true;
      ++i;
    } while (true);
  }
  bool seq(Rows& out, int depth) {
    out.assign(1, Row());
    while (i < t.size() && t[i] != '|' && t[i] != ')') {
      Rows a;
      const bool group = t[i] == '(';
      if (group) {
        if (depth >= kMaxTagLen) return false;
        ops = true;
        ++i;
        if (i < t.size() && t[i] == '?') {
          if (i + 1 >= t.size() || t[i + 1] != ':') return false;
          i += 2;
        }
        if (!alt(a, depth + 1) || i >= t.size() || t[i] != ')') return false;
        ++i;
      } else {
        Elem e;
        if (!parse_elem(t, i, e, wide, extended)) return false;
        a.assign(1, Row(1, e));
      }
      if (extended && i < t.size() && t[i] == '{') {
        if (!counted(a, group)) return false;
      } else if (repeat && i < t.size() && (t[i] == '+' || t[i] == '*')) {
        const int m = t[i] == '+' ? 1 : 0;
        ++i;
        if (!unbounded(a, group, m, m == 0 ? kRepeatRows : m + kRepeatRows - 1)) return false;
      } else if (i < t.size() && t[i] == '?') {  // greedy: present, then absent; "??", "?+", "?*", "?{" are refused
        ops = true;
        ++i;
        if (i < t.size() && std::strchr("?+*{", t[i])) return false;
        add_row(a, Row());
      }
      Rows next;
      for (const Row& l : out)
        for (const Row& r : a) add_row(next, join_rows(l, r));
      out.swap(next);
    }
    return true;
  }
  // "{m}", "{m,n}" or "{,n}" at t[i] == '{' after the atom whose rows are `a` (m <= n <= 61):
  // x{m,n} is m copies of x and n - m nested greedy optionals, x...x(?:x(?:x)?)?, so the rows and
  // their order come from add_row as for '?'.  False for "{m,}", m > n, a quantifier after the
  // '}' and every form re reads as a literal brace ("{", "{x}", "{ 1}", "{}", "{,}").
  static Rows cat(const Rows& l, const Rows& r) {
    Rows out;
    for (const Row& x : l)
      for (const Row& y : r) add_row(out, join_rows(x, y));
    return out;
  }
  // '+', '*' or "{m,}" was read after the atom whose rows are `a`; i is after it.  It expands as
  // x{m, top} does, longest first, and the longest row is open-ended at its last copy of x: "top or
  // more".  Only one element repeats: a group is refused with its own message, a non-ASCII literal
  // (one element per byte), a lazy form and a stacked quantifier with the regex one.  The open-ended
  // copy of a literal is kept as a class of that one letter, so the class walks see the row.
  // (What may follow the run is checked over the whole tag's rows: repeat_overlap.)
  bool unbounded(Rows& a, bool group, int m, int top) {
    if (i < t.size() && std::strchr("?+*{", t[i])) return false;
    if (group) throw TagRefusal{kUnboundedGroup};
    const Elem x = a[0][0];
    if (!x.cls && x.lit >= 0x80) return false;
    ops = true;
    Elem open = x;
    if (!open.cls) {
      open.cls = true;
      tab_set(open.tab, x.lit);
    }
    open.rep = true;
    a.clear();
    for (int n = top; n >= m; --n) {
      if (n > kMaxTagLen) throw RowTooLong();
      Row r((size_t)n, x);
      if (n == top) r.back() = open;
      add_row(a, r);
    }
    return true;
  }
  bool counted(Rows& a, bool group) {
    size_t j = i + 1;
    auto number = [&](int* v) {  // up to three digits ("061" is 61, the largest count); a longer run is refused
      const size_t j0 = j;
      *v = 0;
      while (j < t.size() && t[j] >= '0' && t[j] <= '9' && j - j0 < 3) *v = *v * 10 + (t[j++] - '0');
      return j > j0;
    };
    int m = 0, n = 0;
    const bool has_m = number(&m);
    if (j < t.size() && t[j] == ',') {
      ++j;
      if (repeat && has_m && j < t.size() && t[j] == '}') {  // "{m,}"
        if (m > kMaxTagLen) return false;
        i = j + 1;
        return unbounded(a, group, m, m + kRepeatRows - 1);
      }
      if (!number(&n)) return false;  // "{m,}" is unbounded, "{,}" a literal
    } else {
      if (!has_m) return false;
      n = m;
    }
    if (j >= t.size() || t[j] != '}' || m > n || n > kMaxTagLen) return false;
    ++j;
    if (j < t.size() && std::strchr("?+*{", t[j])) return false;
    for (const Row& r : a)
      if (r.empty()) throw TagRefusal{kEmptyRepeat};  // (re's empty-iteration guard is not the row identity)
    i = j;
    ops = true;
    Rows opt(1, Row());  // the n - m nested optionals, innermost first
    for (int k = 0; k < n - m; ++k) {
      opt = cat(a, opt);
      add_row(opt, Row());
    }
    Rows out(1, Row());
    for (int k = 0; k < m; ++k) out = cat(out, a);
    a = cat(out, opt);
    return true;
  }
};

// The rows of one tag; *ops: it is a variable-width tag.  False outside the subset.
// The overlap rule of unbounded repetition.  X: the class of an open-ended element; F: what stands
// directly after it in a row — the next element, or '>' where the run ends the tag (every follower of
// the quantifier stands after the open-ended copy in some row: the expansion distributes).  Where X
// and F share no character the run takes exactly the maximal run of X characters, the text has at
// most one parse and the quantifier has the matches of the alternation over its counts, in any
// order: what the rows are.  Where they share one the regex backtracks into the run: refused.  The
// ASCII tables are compared as built (under IGNORECASE); two elements that can both take a code
// point >= 0x80 are taken to overlap (the rule errs by refusing only).
bool repeat_overlap(const Rows& rows) {
  for (const Row& r : rows)
    for (size_t i = 0; i < r.size(); ++i) {
      if (!r[i].rep) continue;
      const Elem& x = r[i];
      if (i + 1 == r.size()) {
        if ((x.tab['>' >> 5] >> ('>' & 31)) & 1u) return true;
        continue;
      }
      const Elem& f = r[i + 1];
      const bool xw = (x.flags & (CLS_WIDE | CLS_SH)) != 0;
      if (!f.cls) {
        if (f.lit >= 0x80 ? xw : ((x.tab[f.lit >> 5] >> (f.lit & 31)) & 1u) != 0) return true;
        continue;
      }
      if (xw && (f.flags & (CLS_WIDE | CLS_SH))) return true;
      for (int k = 0; k < 4; ++k)
        if (x.tab[k] & f.tab[k]) return true;
    }
  return false;
}

bool parse_variant_tag(const std::string& t, Rows& out, bool wide, bool extended, bool repeat, bool* ops) {
  VariantParser p{t, wide, extended, repeat};
  if (!p.alt(out, 0) || p.i != t.size()) return false;
  if (repeat && repeat_overlap(out)) throw TagRefusal{kRepeatOverlap};
  *ops = p.ops;
  return true;
}

Tags build_tags(const std::vector<std::string>& tags, bool classes, bool unicode, bool mixed, bool variants,
                bool extended, bool repeat, bool runs, std::vector<std::pair<std::string, int>>* rows_out);

}  // namespace

Tags make_tags(const std::vector<std::string>& tags, bool classes, bool unicode, bool mixed, bool variants,
               bool extended, bool repeat, bool runs) {
  return build_tags(tags, classes, unicode, mixed, variants, extended, repeat, runs, nullptr);
}

std::vector<std::pair<std::string, int>> tagset_rows(const std::vector<std::string>& tags, bool classes, bool unicode,
                                                     bool mixed, bool variants, bool extended, bool repeat, bool runs) {
  std::vector<std::pair<std::string, int>> rows;
  build_tags(tags, classes, unicode, mixed, variants, extended, repeat, runs, &rows);
  return rows;
}

// The case rule of a non-ASCII tag character (qmx_unicode_fold.h, generated from the rule in
// tools/gen_unicode_fold.py).  0: uncased, 1: a pair (*lower: its lower member, which may be
// cp itself), 2: refused.
int unicode_tag_char(uint32_t cp, uint32_t* lower) {
  *lower = cp;
  if (cp < 0x80) return 0;
  for (int k = 0; k < kFoldRefusedCount; ++k)
    if (cp >= kFoldRefused[k][0] && cp <= kFoldRefused[k][1]) return 2;
  for (int k = 0; k < kFoldPairCount; ++k) {
    if (kFoldPairs[k][0] == cp) {
      *lower = kFoldPairs[k][1];
      return 1;
    }
    if (kFoldPairs[k][1] == cp) return 1;
  }
  return 0;
}

uint32_t unicode_tag_partner(uint32_t cp) {
  for (int k = 0; k < kFoldPairCount; ++k) {
    if (kFoldPairs[k][0] == cp) return kFoldPairs[k][1];
    if (kFoldPairs[k][1] == cp) return kFoldPairs[k][0];
  }
  return cp;
}

namespace {
Tags build_tags(const std::vector<std::string>& tags, bool classes, bool unicode, bool mixed, bool variants,
                bool extended, bool repeat, bool runs, std::vector<std::pair<std::string, int>>* rows_out) {
  mixed = mixed && classes && unicode;
  variants = variants && classes;
  extended = extended && variants;
  repeat = repeat && extended;
  runs = runs && repeat;
  Tags out;
  std::memset(&out, 0, sizeof(out));
  TagSet& ts = out.ts;
  TagClasses& tc = out.tc;
  bool any_cls = false, any_wide = false;
  uint32_t pair_tags = 0;  // bit t: tag t holds a pair character
  std::vector<std::string> seen;
  std::vector<Row> row_pat;  // variants: every row's pattern, and the tag it comes from
  std::vector<std::string> row_tag;
  auto pack = [](uint32_t cp, int* len) {  // UTF-8 bytes, byte k at bit 8k
    uint8_t b[4];
    *len = put_wtf8(cp, b);
    uint32_t v = 0;
    for (int k = 0; k < *len; ++k) v |= (uint32_t)b[k] << (8 * k);
    return v;
  };
  for (size_t ti = 0; ti < tags.size(); ++ti) {
    const std::string& t0 = tags[ti];
    std::string t, tw;  // tw: the tag as written, its non-ASCII characters lowered (mixed: the class parser's input)
    bool wide = false, has_pair = false;
    for (char c : t0) wide = wide || (uint8_t)c >= 0x80;
    if (wide && unicode) {
      // a non-ASCII tag: its characters are uncased or one of a simple case pair, lowercased
      // here through the pair table ("É" and "é" are one tag)
      const uint8_t* b = (const uint8_t*)t0.data();
      const int n = (int)t0.size();
      if (!utf8_valid(b, 0, n)) throw std::invalid_argument("tag is not UTF-8: " + t0);
      for (int p = 0; p < n;) {
        uint32_t cp, low;
        p += wtf8_decode(b, p, n, &cp);
        if (cp < 0x80) {
          t.push_back((char)lower_ascii((uint8_t)cp));
          tw.push_back((char)cp);
          continue;
        }
        const int kind = unicode_tag_char(cp, &low);
        if (kind == 2)
          throw std::invalid_argument("tag holds a character without a simple case pair (runs with --impl python): " + t0);
        uint8_t o[4];
        t.append((const char*)o, (size_t)put_wtf8(low, o));
        tw.append((const char*)o, (size_t)put_wtf8(low, o));
        has_pair = has_pair || kind == 1;
        if (kind == 1) {
          int ln;
          const uint32_t lo = pack(low, &ln), up = pack(unicode_tag_partner(low), &ln);
          int f = 0;
          while (f < tc.nfold && tc.fold_lo[f] != lo) ++f;
          if (f == tc.nfold) {
            if (tc.nfold >= kMaxFold) throw std::invalid_argument("too many case-pair characters in the thinking tags (at most 32)");
            tc.fold_lo[f] = lo;
            tc.fold_up[f] = up;
            tc.fold_len[f] = (uint8_t)ln;
            ++tc.nfold;
          }
        }
      }
    } else {
      for (char c : t0) t.push_back((char)lower_ascii((uint8_t)c));
    }
    if (std::find(seen.begin(), seen.end(), t) != seen.end()) continue;
    // regex metacharacters change what quorum's alternation matches (oai_proxy.py:137,
    // 271-274); '<', '>' and '/' in a tag let one tag's pattern start inside another's, so
    // the token model (at most one pattern per '<') would not hold; non-ASCII needs the case
    // rule above (`unicode`).  Everything else is literal, exactly as in the regex.
    bool literal = true;
    for (char ch : t) {
      const uint8_t c = (uint8_t)ch;
      const bool ok = (c >= 0x20 && c < 0x7f && !std::strchr(".^$*+?{}[]\\|()<>/", (int)c)) || (unicode && c >= 0x80);
      if (!ok) literal = false;
    }
    if (t.empty() || (int)t.size() > kMaxTagLen) {
      if (!literal) throw std::invalid_argument("tag needs regex semantics: " + t0);
      throw std::invalid_argument("unsupported tag length: " + t0);
    }
    Rows rows(1);
    bool var = false;  // a variable-width tag: '?', '|' or a group
    if (!literal) {
      // class tags: '.', [...] and escaped punctuation, one code point per element; the
      // tables come from the tag as written (IGNORECASE makes its case immaterial)
      const bool mix = mixed && wide;  // a class element and a non-ASCII literal in one tag
      bool ok = classes;
      if (ok && variants) {
        // (a non-ASCII variable-width tag without `mixed` gets the mixing message below)
        const bool w = wide && unicode;
        rows.clear();
        try {
          ok = parse_variant_tag(w ? tw : t0, rows, w, extended, repeat, &var);
        } catch (const TooManyRows&) {
          throw std::invalid_argument("thinking tags expand to more than 16 rows: " + t0);
        } catch (const RowTooLong&) {
          throw std::invalid_argument("unsupported tag length: " + t0);
        } catch (const TagRefusal& r) {
          throw std::invalid_argument(r.msg + t0);
        }
        // (a shorthand in front gets the class-first message of the rows below)
        if (ok && !var)
          ok = (mix || !wide) && !rows[0].empty() && (!rows[0][0].cls || (rows[0][0].flags & CLS_SH));
      } else if (ok) {
        ok = parse_class_tag(mix ? tw : t0, rows[0], mix);
      }
      if (!ok) throw std::invalid_argument("tag needs regex semantics: " + t0);
      for (const Row& elems : rows) {
        if (elems.empty()) throw std::invalid_argument("tag has an empty alternative: " + t0);
        if (elems[0].cls) throw std::invalid_argument("tag has an alternative that begins with a class: " + t0);
        int bound = 3;  // bytes of the longest "</" + match + ">"
        for (const Elem& e : elems) bound += (e.flags & (CLS_WIDE | CLS_SH)) ? 4 : 1;
        if (bound > kMaxTail) throw std::invalid_argument("unsupported tag length: " + t0);
      }
    }
    seen.push_back(t);
    any_wide = any_wide || wide;  // (a bracket class has ASCII members: every byte >= 0x80 is a literal's)
    any_cls = any_cls || var;     // (its source text is not its pattern: of the class kind)
    for (const Row& elems : rows) {
      if (variants) {
        // the depth-0 holdback keeps ONE source text per pattern: the same pattern from a
        // variable-width tag and from another tag would need both
        Row pat = elems;
        if (literal)
          for (char ch : t) {
            Elem e;
            e.lit = (uint8_t)ch;
            pat.push_back(e);
          }
        for (size_t j = 0; j < row_pat.size(); ++j)
          if (same_row(row_pat[j], pat) && (var || (tc.var >> j) & 1))
            throw std::invalid_argument("two thinking tags give the same pattern under different source texts: " +
                                        row_tag[j] + ", " + t0);
        row_pat.push_back(pat);
        row_tag.push_back(t0);
      }
      if (ts.n >= kMaxTags)
        throw std::invalid_argument(var || tc.var ? "thinking tags expand to more than 16 rows: " + t0
                                                  : std::string("too many thinking tags"));
      if (var) tc.var |= 1u << ts.n;
      if (rows_out) {
        std::string txt = literal ? t : std::string();
        for (const Elem& e : elems) txt += e.rep ? e.txt + "+" : e.txt;  // (open-ended: this element, once or more)
        rows_out->emplace_back(txt, (int)ti);
      }
      if (has_pair) pair_tags |= 1u << ts.n;
      tc.srclen[ts.n] = (int)t.size();
      std::memcpy(tc.src[ts.n], t.data(), t.size());
      if (literal) {
        ts.len[ts.n] = (int)t.size();
        std::memcpy(ts.name[ts.n], t.data(), t.size());
      } else {
        any_cls = true;
        ts.len[ts.n] = (int)elems.size();
        for (size_t i = 0; i < elems.size(); ++i) {
          const Elem& e = elems[i];
          if (!e.cls) {
            ts.name[ts.n][i] = e.lit;
            continue;
          }
          tc.clsmask[ts.n] |= 1ull << i;
          if (e.rep) tc.rep[ts.n] |= 1ull << i;
          int k = 0;
          while (k < tc.n && !(tc.flags[k] == e.flags && std::memcmp(tc.tab[k], e.tab, sizeof(e.tab)) == 0)) ++k;
          if (k == tc.n) {
            if (tc.n >= kMaxClasses) throw std::invalid_argument("too many tag classes");
            std::memcpy(tc.tab[k], e.tab, sizeof(e.tab));
            tc.flags[k] = e.flags;
            ++tc.n;
          }
          ts.name[ts.n][i] = (uint8_t)(0x80 + k);
        }
      }
      ++ts.n;
    }
  }
  if (ts.n == 0) throw std::invalid_argument("empty tag set");
  // a class position is kept as byte 0x80 + k in TagSet::name, where a non-ASCII tag keeps
  // its UTF-8 bytes: only a mixed tag set (`mixed`) tells the two apart, by TagClasses::clsmask
  if (any_cls && any_wide && !mixed)
    throw std::invalid_argument("class tags and non-ASCII tags do not mix in one tag set (runs with --impl python)");
  if (tc.nfold > 0)
    for (int pat = 0; pat < 2 * ts.n; ++pat) tc.span = std::max(tc.span, pattern_len(ts, pat));
  out.kind = any_cls && any_wide ? TAGS_MIXED : tc.nfold > 0 ? TAGS_PAIR : any_cls ? TAGS_CLASS : TAGS_LITERAL;
  if (out.kind == TAGS_MIXED) {
    tc.nfold = -(tc.nfold + 1);  // (mixed_nfold: the kernels tell the three kinds apart by this one word)
    tc.walk = pair_tags;
    for (int t = 0; t < ts.n; ++t)
      if (tc.clsmask[t]) tc.walk |= 1u << t;
  } else {
    std::memset(tc.clsmask, 0, sizeof(tc.clsmask));  // (the tables of the other kinds are what they were)
    tc.walk = 0;
  }
  if (extended && out.kind == TAGS_CLASS) tc.var |= kVarExtended;
  // (a set without an open-ended row has no run to walk: its device tables and paths stay what they were)
  if (runs && (out.kind == TAGS_CLASS || out.kind == TAGS_MIXED))
    for (int t = 0; t < ts.n; ++t)
      if (tc.rep[t]) tc.var |= kVarRuns;
  // (a literal tag set keeps no tables: its source text is its names)
  if (out.kind == TAGS_LITERAL) std::memset(&tc, 0, sizeof(tc));
  return out;
}
}  // namespace

// --------------------------------------------------------------------------------
// streaming filter: state (depth, tail); X = tail ++ text, token walk left to right
// --------------------------------------------------------------------------------
void filter_feed(const Tags& tags, FilterState& fs, const uint8_t* text, size_t n, std::string& out) {
  const TagSet& ts = tags.ts;
  const TagClasses& tc = tags.tc;
  std::string xs;
  xs.reserve(fs.tail_len + n);
  xs.append((const char*)fs.tail, fs.tail_len);
  xs.append((const char*)text, n);
  const uint8_t* x = (const uint8_t*)xs.data();
  int N = (int)xs.size();
  int i = 0;
  fs.tail_len = 0;
  while (true) {
    // next token at or after i (depth 0: opens only are tokens)
    int p = i, tok = 0, L = 0;
    for (; p < N; ++p) {
      if (x[p] != '<') continue;
      tok = token_at(tags.kind, x, N, p, ts, tc, false, &L);
      if (tok > 0 || (tok < 0 && fs.depth > 0)) break;
      tok = 0;
    }
    if (p < N) {
      if (fs.depth == 0) {
        out.append((const char*)x + i, p - i);
        fs.depth = 1;
      } else {
        fs.depth = tok > 0 ? fs.depth + 1 : std::max(fs.depth - 1, 0);
      }
      i = p + L;
      continue;
    }
    // no more tokens: hold back a trailing partial tag from the LAST '<'
    int q = N - 1;
    bool hold;
    if ((tags.kind == TAGS_CLASS || tags.kind == TAGS_MIXED) && fs.depth > 0) {
      // class tags inside a block: a class element may swallow a later '<', so keep from the
      // EARLIEST '<' whose rest is still a proper prefix of some pattern (the reference keeps
      // its whole buffer here; the byte bound of make_tags keeps this within kMaxTail)
      for (q = i; q < N; ++q)
        if (x[q] == '<' && held_at(tags.kind, x, q, N, ts, tc, fs.depth)) break;
      hold = q < N;
    } else {
      while (q >= i && x[q] != '<') --q;
      hold = q >= i && held_at(tags.kind, x, q, N, ts, tc, fs.depth);
    }
    int cut = hold ? q : N;
    if (fs.depth == 0) out.append((const char*)x + i, cut - i);
    if (hold) {
      fs.tail_len = N - q;
      std::memcpy(fs.tail, x + q, fs.tail_len);
    }
    return;
  }
}

// --------------------------------------------------------------------------------
// final strip: tokens, per-tag next-close links, leftmost-first walk, Unicode strip
// --------------------------------------------------------------------------------
// Class tags: re.sub("<(alt)>.*?</\1>", "", I|S) as the backtracking matcher runs it.  At each
// start every alternative is tried in order; its close is the first later "</" + the text the
// open captured + ">" (ASCII case folded, compared with the captured bytes, not the pattern);
// an alternative without a close gives way to the next one.  The closes are indexed once by
// (tag, folded capture) — a text equal to a capture of tag t matches t's elements too — so the
// walk stays near linear where the regex is quadratic.
// A mixed tag set: the same walk over mixed_walk, the capture keys folded through the pair table
// as well (the upper member of one of the set's pair characters stands for its lower member).
static std::string strip_final_classes(const Tags& tags, const uint8_t* x, int n) {
  const TagSet& ts = tags.ts;
  const TagClasses& tc = tags.tc;
  const bool mixed = tags.kind == TAGS_MIXED;
  auto walk = [&](int p, int pat, int* end) {
    return mixed ? mixed_walk(x, n, p, ts, tc, pat, true, end) : class_walk(x, n, p, ts, tc, pat, true, end);
  };
  auto key_of = [&](int t, int a, int b) {
    std::string k(1, (char)t);
    for (int i = a; i < b;) {
      const int ln = mixed ? utf8_lead_len(x[i]) : 1;
      if (ln > 1 && i + ln <= b) {
        uint32_t have = 0;
        for (int j = 0; j < ln; ++j) have |= (uint32_t)x[i + j] << (8 * j);
        for (int f = 0; f < mixed_nfold(tc); ++f)
          if (tc.fold_len[f] == ln && tc.fold_up[f] == have) have = tc.fold_lo[f];
        for (int j = 0; j < ln; ++j) k.push_back((char)(have >> (8 * j)));
        i += ln;
        continue;
      }
      k.push_back((char)lower_ascii(x[i]));
      ++i;
    }
    return k;
  };
  std::unordered_map<std::string, std::vector<int>> closes;  // -> positions of the "</", ascending
  for (int p = 0; p + 1 < n; ++p) {
    if (x[p] != '<' || x[p + 1] != '/') continue;
    for (int t = 0; t < ts.n; ++t) {
      int end = 0;
      if (walk(p, ts.n + t, &end) == 1) closes[key_of(t, p + 2, end - 1)].push_back(p);
    }
  }
  std::string out;
  out.reserve(n);
  int i = 0;
  for (int p = 0; p < n; ++p) {
    if (x[p] != '<') continue;
    for (int t = 0; t < ts.n; ++t) {
      int end = 0;
      if (walk(p, t, &end) != 1) continue;
      auto it = closes.find(key_of(t, p + 1, end - 1));
      if (it == closes.end()) continue;
      auto c = std::lower_bound(it->second.begin(), it->second.end(), end);
      if (c == it->second.end()) continue;
      out.append((const char*)x + i, p - i);
      i = *c + 2 + (end - 1 - (p + 1)) + 1;
      p = i - 1;
      break;
    }
  }
  out.append((const char*)x + i, n - i);
  int a = 0, b = (int)out.size();
  ustrip((const uint8_t*)out.data(), &a, &b);
  return out.substr(a, b - a);
}

std::string strip_final(const Tags& tags, const uint8_t* x, size_t n) {
  const TagSet& ts = tags.ts;
  if (tags.kind == TAGS_CLASS || tags.kind == TAGS_MIXED) return strip_final_classes(tags, x, (int)n);
  // (a pair tag set: the tokens of the folded text — the backreference folds both sides, so a
  // close of the same tag in any case is the open's close, as for ASCII letters)
  struct Tok { int pos, len, id; };
  std::vector<Tok> toks;
  for (int p = 0; p < (int)n; ++p) {
    if (x[p] != '<') continue;
    int L = 0;
    int id = token_at(tags.kind, x, (int)n, p, ts, tags.tc, true, &L);
    if (id != 0) toks.push_back({p, L, id});
  }
  std::vector<int> next_close(toks.size(), -1);
  int last[kMaxTags];
  for (int t = 0; t < kMaxTags; ++t) last[t] = -1;
  for (int k = (int)toks.size() - 1; k >= 0; --k) {
    int id = toks[k].id;
    if (id > 0) next_close[k] = last[id - 1];
    else last[-id - 1] = k;
  }
  std::string out;
  out.reserve(n);
  int i = 0;
  for (int k = 0; k < (int)toks.size(); ++k) {
    if (toks[k].id <= 0 || toks[k].pos < i) continue;
    int j = next_close[k];
    if (j < 0) continue;
    out.append((const char*)x + i, toks[k].pos - i);
    i = toks[j].pos + toks[j].len;
    k = j;
  }
  out.append((const char*)x + i, n - i);
  int a = 0, b = (int)out.size();
  ustrip((const uint8_t*)out.data(), &a, &b);
  return out.substr(a, b - a);
}

// --------------------------------------------------------------------------------
// SSE encoding
// --------------------------------------------------------------------------------
size_t escaped_size(const uint8_t* y, size_t n) {
  size_t s = 0;
  for (size_t p = 0; p < n;) {
    uint32_t cp;
    p += wtf8_decode(y, (int)p, (int)n, &cp);
    s += escaped_len_cp(cp);
  }
  return s;
}
void escape_append(const uint8_t* y, size_t n, std::string& out) {
  uint8_t buf[12];
  for (size_t p = 0; p < n;) {
    uint32_t cp;
    p += wtf8_decode(y, (int)p, (int)n, &cp);
    int k = escape_cp(cp, buf);
    out.append((const char*)buf, k);
  }
}
static void delta_prefix_append(int index, int64_t created, std::string& out) {
  char b[224];
  const int n = snprintf(b, sizeof(b),
                         "data: {\"id\": \"chatcmpl-parallel-%d\", \"object\": \"chat.completion.chunk\", "
                         "\"created\": %lld, \"model\": \"parallel-proxy\", \"choices\": [{\"index\": 0, "
                         "\"delta\": {\"content\": \"",
                         index, (long long)created);
  out.append(b, (size_t)n);
}
std::string delta_prefix(int index, int64_t created) {
  std::string s;
  delta_prefix_append(index, created, s);
  return s;
}
std::string final_prefix(int64_t created) {
  return "data: {\"id\": \"chatcmpl-parallel-final\", \"object\": \"chat.completion.chunk\", \"created\": " +
         std::to_string(created) +
         ", \"model\": \"parallel-proxy\", \"choices\": [{\"index\": 0, \"delta\": {\"content\": \"";
}

// --------------------------------------------------------------------------------
// per-stream processing (sequential)
// --------------------------------------------------------------------------------
// Is x[a:b) a complete JSON string body (valid escapes, no control characters, no unescaped
// quote, strict UTF-8)?  The template fast path of the CPU engine (the HIP kernel's
// wave_str_body, sequentially).
static bool str_body_ok(const uint8_t* x, int a, int b) {
  for (int p = a; p < b; ++p) {
    const uint8_t c = x[p];
    if (c == '"' || c < 0x20) return false;
    if (c == '\\') {
      if (++p >= b) return false;
      const uint8_t d = x[p];
      if (d == 'u') {
        if (p + 4 >= b) return false;
        for (int k = 1; k <= 4; ++k)
          if (hexv(x[p + k]) < 0) return false;
        p += 4;
      } else if (!(d == '"' || d == '\\' || d == '/' || d == 'b' || d == 'f' || d == 'n' || d == 'r' || d == 't')) {
        return false;
      }
    }
  }
  return utf8_valid(x, a, b);
}

static void handle_event(const Tags& tags, SlotCore& s, const uint8_t* e, int m, int64_t created,
                         std::string& out, std::string& scratch) {
  EvResult r;
  const int tp = (int)s.tpl_pre.size(), tsz = (int)s.tpl_suf.size();
  if (tp > 0 && m >= tp + tsz && std::memcmp(e, s.tpl_pre.data(), tp) == 0 &&
      std::memcmp(e + m - tsz, s.tpl_suf.data(), tsz) == 0 && str_body_ok(e, tp, m - tsz)) {
    r.kind = EV_CONTENT;  // same shape as this stream's last parsed content event
    r.str_a = tp;
    r.str_b = m - tsz;
  } else {
    r = classify_event(e, m);
    if (r.kind == EV_CONTENT && r.str_a <= 256 && m - r.str_b <= 64) {
      s.tpl_pre.assign((const char*)e, r.str_a);
      s.tpl_suf.assign((const char*)e + r.str_b, m - r.str_b);
    }
  }
  if (r.kind == EV_SKIP) return;
  if (r.kind == EV_ABORT) {
    s.aborted = true;
    return;
  }
  const int dl = json_unescape(e, r.str_a, r.str_b, nullptr);
  thread_local std::string c;  // unescaped content (reused: no allocation per event)
  c.resize((size_t)dl);
  json_unescape(e, r.str_a, r.str_b, (uint8_t*)&c[0]);
  scratch.clear();
  if (s.filter) filter_feed(tags, s.fs, (const uint8_t*)c.data(), c.size(), scratch);
  else scratch.assign(c);
  s.content += scratch;
  if (!scratch.empty() && s.emit) {
    delta_prefix_append(s.index, created, out);
    escape_append((const uint8_t*)scratch.data(), scratch.size(), out);
    out += kDeltaSuffix;
  }
}

void process_slot(const Tags& tags, SlotCore& s, const uint8_t* data, size_t n, bool eof, int64_t created,
                  std::string& out) {
  if (s.aborted || s.done) return;
  s.carry.append((const char*)data, n);
  const uint8_t* x = (const uint8_t*)s.carry.data();
  int N = (int)s.carry.size();
  int pos = 0;
  if (!s.started) {
    while (pos < N) {
      int w = ws_at(x, pos, N);
      if (w <= 0) break;
      pos += w;
    }
    bool undecided = pos < N && ws_at(x, pos, N) < 0;
    if (pos >= N || (undecided && !eof)) {
      s.carry.erase(0, pos);
      if (eof) s.done = true;
      return;
    }
    s.started = true;
  }
  thread_local std::string scratch;
  int from = pos;  // no separator starts before `from` (memchr for '\n', then check the next byte)
  while (!s.aborted) {
    const void* nl = from < N ? memchr(x + from, '\n', (size_t)(N - from)) : nullptr;
    if (!nl) break;
    const int j = (int)((const uint8_t*)nl - x);
    if (j + 1 >= N) break;
    if (x[j + 1] != '\n') {
      from = j + 1;
      continue;
    }
    handle_event(tags, s, x + pos, j - pos, created, out, scratch);  // leftmost separator
    pos = from = j + 2;
  }
  if (s.aborted) {
    s.carry.clear();
    return;
  }
  if (eof) {
    if (pos < N) handle_event(tags, s, x + pos, N - pos, created, out, scratch);
    s.carry.clear();
    if (!s.aborted) s.done = true;
    return;
  }
  s.carry.erase(0, pos);
}

void finalize_texts(const Tags& tags, const std::vector<std::string>& texts, const FinalizeReq& r,
                    FinalizeRes& out) {
  out.id = r.id;
  std::vector<std::string> kept;
  for (const auto& t : texts) {
    if (t.empty()) continue;
    kept.push_back(r.strip ? strip_final(tags, (const uint8_t*)t.data(), t.size()) : t);
  }
  if (r.texts) {
    out.kind = 2;
    out.texts = std::move(kept);
    return;
  }
  if (kept.empty()) {
    out.kind = 0;
    return;
  }
  std::string joined;
  for (size_t i = 0; i < kept.size(); ++i) {
    if (i) joined += r.joiner;
    joined += kept[i];
  }
  out.kind = 1;
  out.event = final_prefix(r.created);
  escape_append((const uint8_t*)joined.data(), joined.size(), out.event);
  out.event += kFinalSuffix;
}

// --------------------------------------------------------------------------------
// HostEngine
// --------------------------------------------------------------------------------
static double mono_s() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

HostEngine::HostEngine(const Tags& tags) : tags_(tags) {
  if (const char* pe = env_get("QMX_PIPELINE")) pipeline_ = atoi(pe) != 0;
}

int HostEngine::open(int index, bool filter, bool emit, uint32_t* gen) {
  std::lock_guard<std::mutex> g(mu_);
  int slot;
  if (!free_.empty()) {
    slot = free_.back();
    free_.pop_back();
  } else {
    slot = (int)meta_.size();
    meta_.emplace_back();
    core_.emplace_back();
  }
  open_reserved(slot, index, filter, emit, gen);
  return slot;
}

void HostEngine::reserve(int k, std::vector<int>& out) {
  std::lock_guard<std::mutex> g(mu_);
  for (int i = 0; i < k; ++i) {
    if (!free_.empty()) {
      out.push_back(free_.back());
      free_.pop_back();
    } else {
      out.push_back((int)meta_.size());
      meta_.emplace_back();
      core_.emplace_back();
    }
  }
}

void HostEngine::open_reserved(int slot, int index, bool filter, bool emit, uint32_t* gen) {
  // reset in place: a reused slot keeps its (small) buffers, so a new session costs no
  // allocation under the engine lock
  auto recycle = [](std::string& x) {
    if (x.capacity() > (64u << 10)) std::string().swap(x);
    else x.clear();
  };
  Meta& m = meta_[slot];
  m.gen += 1;
  m.live = true;
  m.dirty = m.eof = m.closed = m.busy = false;
  m.fresh = true;
  recycle(m.incoming);
  if (gen) *gen = m.gen;
  SlotCore& c = core_[slot];
  c.filter = filter;
  c.emit = emit;
  c.started = c.aborted = c.done = false;
  c.index = index;
  recycle(c.carry);
  c.fs = FilterState();
  recycle(c.content);
  recycle(c.tpl_pre);
  recycle(c.tpl_suf);
}

void HostEngine::feed(int slot, const std::string& data) {
  std::lock_guard<std::mutex> g(mu_);
  feed_locked(slot, data);
}

void HostEngine::finish(int slot) {
  std::lock_guard<std::mutex> g(mu_);
  finish_locked(slot);
}

void HostEngine::release(int slot) {
  std::lock_guard<std::mutex> g(mu_);
  release_locked(slot);
}

void HostEngine::apply_ops(std::vector<EngineOp>& ops, bool move_data) {
  std::lock_guard<std::mutex> g(mu_);
  for (auto& op : ops) {
    if (op.kind == EngineOp::FEED) {
      if (move_data) feed_locked_move(op.slot, op.data);
      else feed_locked(op.slot, op.data);
    }
    else if (op.kind == EngineOp::FINISH) finish_locked(op.slot);
    else release_locked(op.slot);
  }
}

void HostEngine::feed_locked(int slot, const std::string& data) {
  if (slot < 0 || slot >= (int)meta_.size() || !meta_[slot].live) return;
  Meta& m = meta_[slot];
  m.incoming += data;
  bytes_in_ += data.size();
  if (!m.dirty) {
    m.dirty = true;
    m.t_dirty = mono_s();
    dirty_.push_back(slot);
  }
}

// Same as feed_locked, but an empty backlog takes the payload's buffer instead of a copy
// (the common case: the previous tick consumed everything), shortening the lock hold.
void HostEngine::feed_locked_move(int slot, std::string& data) {
  if (slot < 0 || slot >= (int)meta_.size() || !meta_[slot].live) return;
  if (!meta_[slot].incoming.empty()) return feed_locked(slot, data);
  bytes_in_ += data.size();
  meta_[slot].incoming.swap(data);
  Meta& m = meta_[slot];
  if (!m.dirty) {
    m.dirty = true;
    m.t_dirty = mono_s();
    dirty_.push_back(slot);
  }
}

void HostEngine::finish_locked(int slot) {
  if (slot < 0 || slot >= (int)meta_.size() || !meta_[slot].live) return;
  Meta& m = meta_[slot];
  m.eof = true;
  if (!m.dirty) {
    m.dirty = true;
    m.t_dirty = mono_s();
    dirty_.push_back(slot);
  }
}

void HostEngine::release_locked(int slot) {
  if (slot < 0 || slot >= (int)meta_.size() || !meta_[slot].live) return;
  meta_[slot].live = false;
  meta_[slot].incoming.clear();
  pending_free_.push_back(slot);
}

int HostEngine::submit_finalize(const std::vector<int>& slots, bool strip, bool texts, const std::string& joiner,
                                int64_t created) {
  std::lock_guard<std::mutex> g(mu_);
  FinalizeReq r{++next_fid_, slots, strip, texts, joiner, created};
  fin_.push_back(std::move(r));
  return next_fid_;
}

bool HostEngine::has_work() {
  std::lock_guard<std::mutex> g(mu_);
  if (!fin_.empty()) return true;
  for (int s : dirty_)
    if (!meta_[s].busy) return true;
  return false;
}

bool HostEngine::pending(int slot) {
  std::lock_guard<std::mutex> g(mu_);
  if (slot < 0 || slot >= (int)meta_.size()) return false;
  const Meta& m = meta_[slot];
  return m.live && (m.dirty || m.busy || !m.incoming.empty());
}

bool HostEngine::job_take(Job& j, bool allow_fin) {
  j.work.clear();
  j.fin.clear();
  thread_local std::vector<int> keep;
  keep.clear();
  std::lock_guard<std::mutex> g(mu_);
  for (int s : pending_free_) {
    if (meta_[s].busy) {  // still in flight on another lane: free it once settled
      keep.push_back(s);
      continue;
    }
    on_free(s);
    free_.push_back(s);
  }
  pending_free_.swap(keep);
  keep.clear();
  j.work.reserve(dirty_.size());
  double now = 0;
  for (int s : dirty_) {
    Meta& m = meta_[s];
    if (m.busy && m.live) {  // this stream's previous tick is not settled: next time
      keep.push_back(s);
      continue;
    }
    m.dirty = false;
    if (!m.live) continue;
    if (m.t_dirty > 0) {
      if (now == 0) now = mono_s();
      take_wait_s_ += now - m.t_dirty;
      ++takes_;
    }
    Work w{s, std::string(), m.eof, m.fresh};
    w.data.swap(m.incoming);
    m.fresh = false;
    m.busy = true;
    j.work.push_back(std::move(w));
  }
  dirty_.swap(keep);
  if (allow_fin) j.fin.swap(fin_);
  if (!j.work.empty() || !j.fin.empty()) ++ticks_;
  return !j.work.empty() || !j.fin.empty();
}

void HostEngine::job_finish(Job& j, std::vector<SlotResult>& results, std::vector<int>& taken) {
  size_t out = 0;
  for (auto& r : results) out += r.size();
  for (auto& w : j.work) taken.push_back(w.slot);
  std::lock_guard<std::mutex> g(mu_);
  bytes_out_ += out;
  // a taken slot stays busy until settled, so it cannot be re-opened meanwhile: its
  // generation is the one the results belong to
  for (auto& r : results) r.gen = meta_[r.slot].gen;
}

bool HostEngine::tick(int64_t created, std::vector<SlotResult>& results, std::vector<FinalizeRes>& fres, int lane,
                      std::vector<int>* taken) {
  // per-thread scratch reused from tick to tick (a tick thread drives one lane)
  thread_local Job j;
  thread_local std::vector<int> slots;
  slots.clear();
  if (!job_take(j, true)) return false;
  run_tick(j.work, j.fin, created, results, fres, lane);
  std::vector<int>& tk = taken ? *taken : slots;
  job_finish(j, results, tk);
  if (!taken) settle(slots);
  return true;
}

void HostEngine::settle(const std::vector<int>& taken) {
  std::lock_guard<std::mutex> g(mu_);
  for (int s : taken) meta_[s].busy = false;
}

std::string HostEngine::text(int slot) {
  if (slot < 0 || slot >= (int)nslots()) return std::string();
  const SlotCore& c = core_[slot];
  return c.aborted ? std::string() : c.content;
}

size_t HostEngine::content_size(int slot) {
  if (slot < 0 || slot >= (int)nslots()) return 0;
  return core_[slot].content.size();
}

void HostEngine::set_remote_content(int slot, const std::string* bytes, size_t len, bool /*host_copied*/) {
  if (slot < 0 || slot >= (int)nslots()) return;
  core_[slot].content = bytes ? *bytes : std::string(len, '\0');
}

std::unordered_map<std::string, double> HostEngine::stats() {
  std::lock_guard<std::mutex> g(mu_);
  return {{"ticks", (double)ticks_}, {"bytes_in", (double)bytes_in_}, {"bytes_out", (double)bytes_out_},
          {"takes", (double)takes_}, {"take_wait_us", take_wait_s_ * 1e6},
          {"slots", (double)meta_.size()}, {"free", (double)free_.size()}};
}

// --------------------------------------------------------------------------------
// CpuEngine
// --------------------------------------------------------------------------------
void CpuEngine::run_tick(std::vector<Work>& work, std::vector<FinalizeReq>& fin, int64_t created,
                         std::vector<SlotResult>& results, std::vector<FinalizeRes>& fres, int /*lane*/) {
  for (auto& w : work) {
    SlotCore& c = core_[w.slot];
    bool was_closed = c.done || c.aborted;
    std::string out;
    process_slot(tags_, c, (const uint8_t*)w.data.data(), w.data.size(), w.eof, created, out);
    int flags = (c.done ? RF_DONE : 0) | (c.aborted ? RF_ABORTED : 0);
    if (!out.empty() || (flags && !was_closed)) results.push_back({w.slot, std::move(out), flags});
  }
  for (auto& r : fin) {
    std::vector<std::string> texts;
    for (int s : r.slots) texts.push_back(text(s));
    FinalizeRes fr;
    finalize_texts(tags_, texts, r, fr);
    fres.push_back(std::move(fr));
  }
}

}  // namespace qmx

namespace qmx {

struct AsyncCpuEngine::Done {
  std::vector<SlotResult> results;
  std::vector<FinalizeRes> fres;
  std::atomic<bool> ready{false};
};

AsyncCpuEngine::AsyncCpuEngine(const Tags& tags) : CpuEngine(tags) {
  th_ = std::thread([this] { run(); });
}

AsyncCpuEngine::~AsyncCpuEngine() {
  {
    std::lock_guard<std::mutex> g(qmu_);
    stop_ = true;
  }
  qcv_.notify_all();
  if (th_.joinable()) th_.join();
}

void AsyncCpuEngine::job_post(Job& j) {
  auto d = std::make_shared<Done>();
  j.impl = d;
  inflight_.fetch_add(1, std::memory_order_acq_rel);
  {
    std::lock_guard<std::mutex> g(qmu_);
    q_.push_back(&j);
  }
  qcv_.notify_one();
}

void AsyncCpuEngine::run() {
  for (;;) {
    Job* j = nullptr;
    {
      std::unique_lock<std::mutex> lk(qmu_);
      qcv_.wait(lk, [this] { return stop_ || !q_.empty(); });
      if (q_.empty()) return;  // stopping with nothing queued
      j = q_.front();
      q_.erase(q_.begin());
    }
    auto d = std::static_pointer_cast<Done>(j->impl);
    run_tick(j->work, j->fin, j->created, d->results, d->fres, 0);
    d->ready.store(true, std::memory_order_release);
  }
}

bool AsyncCpuEngine::job_ready(Job& j, double* expect_us) {
  if (expect_us) *expect_us = 5.0;
  auto d = std::static_pointer_cast<Done>(j.impl);
  return !d || d->ready.load(std::memory_order_acquire);
}

void AsyncCpuEngine::job_complete(Job& j, std::vector<SlotResult>& results, std::vector<FinalizeRes>& fres) {
  auto d = std::static_pointer_cast<Done>(j.impl);
  if (!d) return;  // never posted
  for (auto& r : d->results) results.push_back(std::move(r));
  for (auto& f : d->fres) fres.push_back(std::move(f));
  j.impl.reset();
  inflight_.fetch_sub(1, std::memory_order_acq_rel);
}

}  // namespace qmx
