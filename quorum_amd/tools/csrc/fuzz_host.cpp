// qmx_fuzz_host — host-code fuzzer for the native runtime, built with ASan + UBSan
// (sanitizer builds of the C++ host runtime; GPU sanitizers are not used).
//
// Properties checked on random inputs (no python in the loop):
//  * streaming invariance: the C++ CPU engine produces byte-identical SSE output, flags,
//    content and finals whether a stream is fed in one piece or split at random points with
//    ticks at random moments (the tile/carry/holdback logic of every split point) — with the
//    default tags and with class tag sets ('.', "[...]", escapes: make_tags(tags, true)),
//    their pieces including multi-byte code points and '<' / '>' at class positions, and with
//    non-ASCII tag sets (make_tags(tags, false, true): uncased and case-pair characters, the
//    text folded on read), their pieces in both cases, look-alikes and JSON-escaped forms,
//    and with mixed tag sets (make_tags(tags, true, true, true): class elements and non-ASCII
//    literals in one set and in one tag), and with variable-width tag sets (make_tags(tags, true,
//    ..., true): '?', '|' and groups, every tag its rows), their pieces every row in both cases,
//    the source texts cut short, '>' and non-ASCII at the optional class positions;
//  * malformed tags: random strings over the tag grammar's alphabet — unbalanced '(', a trailing
//    '|', "(?", a depth of 100 among them — fed to make_tags with every key on either are accepted
//    or throw std::invalid_argument, and never crash (the parser is recursive code over user input);
//  * strip_final idempotence on already-stripped text and JSON DOM round-trips
//    (parse(dump(parse(x))) == parse(x)), py_float_repr/escape on random inputs;
//  * everything runs under -fsanitize=address,undefined: any OOB / UB aborts the run.
//
//   qmx_fuzz_host [iterations] [seed]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "qmx_engine.h"
#include "qmx_json.h"

using namespace qmx;

namespace {

std::mt19937_64 rng;
int R(int n) { return (int)(rng() % (uint64_t)n); }

const char* kPieces[] = {"<think>", "</think>", "<THINK>", "</Think>", "<reason>", "</reason>", "<thi", "nk>", "</",
                         "<", ">", "x", "hello ", " ", "\n", "\\n", "\\\"", "\\\\", "\\u00e9", "\\ud83d\\ude00",
                         "\xc3\xa9", "\xe4\xb8\xad", "\xf0\x9f\x98\x80", "\\u0000", "\t", "0"};

// class tag sets and pieces that instantiate them (JSON string bodies, as kPieces)
struct ClassSet {
  std::vector<std::string> tags;
  std::vector<const char*> pieces;
  bool unicode = false;  // a non-ASCII tag set (make_tags' `unicode`), no class tags
  bool mixed = false;    // a mixed tag set (make_tags' `classes`, `unicode` and `mixed`)
  bool variants = false;  // variable-width tags (make_tags' `variants`, with `classes`)
  bool extended = false;  // shorthands and counted repetition (make_tags' `extended`, with `variants`)
  bool repeat = false;    // '+', '*' and "{m,}" after one element (make_tags' `repeat`, with `extended`)
};
const ClassSet kClassSets[] = {
    {{"think", "th.nk"},
     {"<thXnk>", "</th-nk>", "<TH.NK>", "<th", "Xnk>", ".nk>", "</th", "<th\xe4\xb8\xadnk>", "</th\\u4e2dnk>",
      "<th\xf0\x9f\x98\x80nk>", "<th\\ud83d\\ude00nk>", "<th<nk>", "<th>nk>", "<th\\nnk>", "</thXnk>", "<think>", "</think>"}},
    {{"t[0-9][0-9]", "note\\.x", "n[a-c-]te", "x[^y]z"},
     {"<t42>", "</T07>", "<t4", "2>", "<tx2>", "<note.x>", "</NOTE.X>", "<noteQx>", "<note\\\\.", "x>", "<n-te>", "</nBte>",
      "<ndte>", "<xQz>", "</x\xc3\xa9z>", "<x<z>", "<x>z>", "<xyz>", "<x\\nz>", "</x", "z>"}},
    {{"a.", "a", "q[^a-z]"},
     {"<a>", "<a>>", "</a>>", "</a>", "<aX>", "</A\xe4\xb8\xad>", "<q1>", "</q\xf0\x9f\x98\x80>", "<qa>", "<q<>", "<q", "<a"}},
    // a pair tag set (réflexion, я, 𐐨x) with the uncased 思考
    {{"think", "réflexion", "я", "𐐨x", "思考"},
     {"<réflexion>", "</RÉFLEXION>", "<R\\u00c9flexion>", "<rèflexion>", "<RÉ", "flexion>", "<я>", "</Я>", "<ю>", "<\\u042f>",
      "<𐐀X>", "</𐐨x>", "<\\ud801\\udc00x>", "<\\ud801", "\\udc00x>", "<思考>", "</\\u601d\\u8003>", "<思", "考>", "<怞考>",
      "<think>", "</THINK>"},
     true},
    // an uncased (literal) set with a pattern past the 16-byte window
    {{"思考", "a思考过程分"},
     {"<思考>", "</思考>", "<a思考过程分>", "</A思考过程分>", "</a思考过程切>", "<a思考", "过程分>", "<\\u601d", "\\u8003>"},
     true},
    // mixed tag sets: class and pair in separate tags; both in one tag, a non-ASCII first element
    {{"think", "réflexion", "t[0-9]", "思考"},
     {"<réflexion>", "</RÉFLEXION>", "<R\\u00c9flexion>", "<rèflexion>", "<RÉ", "flexion>", "<t4>", "</T7>", "<t", "4>", "<tx>",
      "<t\xc3\xa9>", "<t<>", "<t>>", "<思考>", "</\\u601d\\u8003>", "<思", "考>", "<think>", "</THINK>"},
     true, true},
    {{"réfl.xion", "思[0-9]", "é.", "abcdefghijklmn.я"},
     {"<réfl0xion>", "</RÉFL0XION>", "<R\\u00c9FLxXION>", "<réfl.xion>", "<réfl", "0xion>", ".xion>", "<réfl\xc3\xa9xion>",
      "</réfl\xc3\x89xion>", "<réfl<xion>", "<réfl>xion>", "<réfl\\nxion>", "<思7>", "</思8>", "<思", "7>", "<思\xc3\xa9>", "<怞7>",
      "<é1>", "</É1>", "<é>>", "</é\xe4\xb8\xad>", "<\\u00c9", "x>", "<abcdefghijklmn7я>", "</ABCDEFGHIJKLMNxЯ>",
      "<abcdefghijklmn", ".я>", "7\\u042f>", "<abcdefghijklmn\xe4\xb8\xadя>"},
     true, true},
    // variable-width tags: optional letters and groups, an optional class element, '|'
    {{"think(ing)?", "thoughts?", "t[0-9]?"},
     {"<think>", "</THINKING>", "<thinking>", "</think>", "<thinki", "ng>", "<think(ing)?>", "<think(ing", "<thoughts>",
      "</thought>", "<THOUGHT>", "</Thoughts>", "<thought", "s>", "<t>", "</t>", "<t7>", "</T7>", "<t>>", "<t<>", "<té>",
      "<t\\n>", "<t[0-9]?>", "<t", "7>"},
     false, false, true},
    {{"step[0-9]?|phase", "a(b|c.)?d", "abcdefghijklmno?p"},
     {"<step>", "</STEP4>", "<step4>", "<phase>", "</Phase>", "<step|phase>", "<ste", "p>", "<abd>", "</ACXD>", "<ad>", "<ac>d>",
      "</ac中d>", "<ac<d>", "<a(b|c.)?d>", "<abcdefghijklmnop>", "</ABCDEFGHIJKLMNP>", "<abcdefghijklmnoq>",
      "<abcdefghijklmn", "op>", "p>"},
     false, false, true},
    {{"réflexions?", "思(考)?", "é[0-9]?"},
     {"<réflexion>", "</RÉFLEXIONS>", "<R\\u00c9flexions>", "<réflexions?>", "<réflexion", "s>", "<思>", "</思考>", "<思(考)?>",
      "<\\u601d", "考>", "<é>", "</É7>", "<é>>", "<éé>", "<é", "7>"},
     true, true, true},
    // extended tags: shorthands (a non-ASCII digit, space or letter at their positions, whole and cut
    // inside the code point) and counted repetition
    {{"step\\d", "t\\d?", "h[1-6]{1,2}", "sec\\s\\d{1,3}", "n[\\w-]{2}"},
     {"<step1>", "</STEP1>", "<step\xd9\xa3>", "</step\xd9\xa3>", "<step\\u0663>", "<step\xef\xbc\x93>", "<step", "1>", "\xd9\xa3>",
      "<step\\\\d>", "<step\\\\", "<stepx>", "<step<>", "<t>", "</t>", "<t5>", "</T5>", "<t\xd9\xa3>", "<t>>", "<h1>", "</H16>", "<h12>",
      "<h7>", "<h123>", "<h", "<sec 1>", "</SEC\\n12>", "<sec\xc2\xa0" "7>", "<sec\xe3\x80\x80" "123>", "<sec 1234>", "<sec\\t", "<nab>",
      "</N-_>", "<n\xc3\xa9\xe6\x80\x9d>", "</n\xc3\xa9\xe6\x80\x9d>", "<n\xc3\x89\xe6\x80\x9d>", "<n\xc3\xa9", "<na>", "<n<b>"},
     false, false, true, true},
    {{"\xe6\x80\x9d\\d", "r\xc3\xa9" "fl\\w{1,2}"},
     {"<\xe6\x80\x9d" "7>", "</\xe6\x80\x9d" "7>", "<\xe6\x80\x9d\xd9\xa3>", "</\xe6\x80\x9d\xd9\xa3>", "<\xe6\x80\x9d", "7>", "\xd9\xa3>",
      "<\xe6\x80\x9d\\\\d>", "<r\xc3\xa9" "flx>", "</R\xc3\x89" "FLXY>", "<r\xc3\xa9" "fl\xc3\xa9>", "</r\xc3\xa9" "fl\xc3\xa9>",
      "<r\xc3\xa9" "fl\xe6\x80\x9d" "1>", "<r\xc3\xa9" "fl", "x>", "<r\xc3\xa9" "fl >", "<r\xc3\xa9" "fl<>"},
     true, true, true, true},
    // unbounded repetition: runs inside and beyond the rows, a run up to and past the 61-byte bound,
    // a non-ASCII digit inside a run (whole and cut inside the code point), a repeated literal
    {{"step\\d+", "think\\s*", "hm+"},
     {"<step1>", "</STEP12>", "<step1234>", "<step12345>", "</step12345>", "<step123456789012>", "<step", "12", "345>", ">",
      "<step>", "<stepx>", "<step1\xd9\xa3" "2>", "</step1\xd9\xa3" "2>", "<step12\xd9", "<step\\\\d+>", "<step\\\\d",
      "<step12345678901234567890123456789012345678901234567890123456", "7", "8>", "</step1234567890123456789012345678901234567890123456789012345",
      "67>", "<think>", "<think >", "</THINK \\n\\t  >", "<think      >", "<think\xc2\xa0>", "<think\xe3\x80\x80 >", "<hm>", "</HMMM>",
      "<hmmmmmmm>", "</hmmmmmmm>", "<hmm", "mm>", "<h>"},
     false, false, true, true, true},
    {{"v\\d+\\.\\d+"},
     {"<v1.2>", "</V12.345>", "<v12345.67890>", "</v12345.67890>", "<v1.>", "<v.1>", "<v1", ".2>", "23", "<v1\xd9\xa3.4>", "<v1.2.3>",
      "<v1234567890123456789012345678901234567890123456789012345678.", "5", "5>", "<v\\\\d+"},
     false, false, true, true, true},
    {{"\xe6\x80\x9d\\d+", "r\xc3\xa9" "fl\\w*", "a{2,}b"},
     {"<\xe6\x80\x9d" "7>", "</\xe6\x80\x9d" "7>", "<\xe6\x80\x9d" "12345>", "</\xe6\x80\x9d" "12345>", "<\xe6\x80\x9d\xd9\xa3" "1>",
      "<\xe6\x80\x9d", "12", "345>", "<\xe6\x80\x9d>", "<\xe6\x80\x9d\\\\d+>", "<r\xc3\xa9" "fl>", "</R\xc3\x89" "FLABCDEF>",
      "<r\xc3\xa9" "fl\xc3\xa9\xe6\x80\x9d_1>", "<r\xc3\xa9" "fl", "abc", "defg>", "<r\xc3\xa9" "fl >",
      "<aab>", "</AAAAAAB>", "<ab>", "<aa", "ab>", "<aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaab>"},
     true, true, true, true, true},
};
const ClassSet* g_class = nullptr;  // the class tag set of this iteration (null: the default tags)
constexpr int kClassSetCount = (int)(sizeof(kClassSets) / sizeof(kClassSets[0]));
// The sets with unbounded repetition run a second time with make_tags' `runs` (the kernels' rule for a
// run longer than the rows, qmx_text.h WALK_RUNS): the host engines' bytes must not depend on it.
int repeat_set(int k) {  // the k-th set with `repeat`, counted round
  int nrep = 0;
  for (const ClassSet& c : kClassSets) nrep += c.repeat;
  k %= nrep;
  for (int i = 0; i < kClassSetCount; ++i)
    if (kClassSets[i].repeat && k-- == 0) return i;
  return 0;
}
int repeat_sets() {
  int nrep = 0;
  for (const ClassSet& c : kClassSets) nrep += c.repeat;
  return nrep;
}

// The kernels' candidate rule on the host (device_token_at) against the exact walk (token_at): at
// every '<' of a text the rule either leaves the candidate to the host (suspect) or answers the exact
// walk's token and byte length, with the streaming and with the strip tables.
bool device_rule_holds(const Tags& tags, const std::string& text) {
  const uint8_t* x = (const uint8_t*)text.data();
  const int n = (int)text.size();
  for (int strip = 0; strip < 2; ++strip)
    for (int p = 0; p < n; ++p) {
      if (x[p] != '<') continue;
      int tok = 0, len = 0, want_len = 0;
      const int r = device_token_at(tags.kind, x, n, p, tags.ts, tags.tc, strip != 0, &tok, &len);
      if (r == CC_SUSPECT) continue;
      const int want = token_at(tags.kind, x, n, p, tags.ts, tags.tc, strip != 0, &want_len);
      if (tok != want || (want != 0 && len != want_len)) return false;
    }
  return true;
}

std::string rand_content() {
  std::string s;
  int n = R(12);
  for (int i = 0; i < n; ++i) {
    if (g_class != nullptr && R(2)) s += g_class->pieces[R((int)g_class->pieces.size())];
    else s += kPieces[R(sizeof(kPieces) / sizeof(kPieces[0]))];
  }
  return s;
}

std::string rand_event() {
  switch (R(14)) {
    case 0: return "data: [DONE]\n\n";
    case 1: return "data: {\"choices\": [{\"delta\": {\"content\": null}}]}\n\n";
    case 2: return "event: ping\n\n";
    case 3: return "data: {bad json\n\n";
    case 4: return "data: {\"choices\": []}\n\n";
    case 5: return "data: {\"choices\": [{\"delta\": {\"role\": \"assistant\"}}]}\n\n";
    case 6: return "data: \xff\xfe\n\n";
    default: break;
  }
  std::string c = rand_content();
  std::string ev = "data: {\"id\": \"x\", \"choices\": [{\"index\": 0, \"delta\": {\"content\": \"" + c +
                   "\"}, \"finish_reason\": null}]}\n\n";
  if (R(10) == 0) ev.insert(6, "  ");
  return ev;
}

struct Run {
  std::vector<std::string> sse;
  std::vector<int> flags;
  std::vector<std::string> text;
  std::string fin_event;
  std::vector<std::string> fin_texts;
};

Run run_engine(const Tags& tags, const std::vector<std::string>& bodies, const std::vector<bool>& filt, bool split) {
  CpuEngine eng(tags);
  Run out;
  std::vector<int> slots;
  for (size_t i = 0; i < bodies.size(); ++i) slots.push_back(eng.open((int)i, filt[i], true));
  out.sse.assign(bodies.size(), std::string());
  out.flags.assign(bodies.size(), 0);
  std::vector<size_t> pos(bodies.size(), 0);
  std::vector<SlotResult> r;
  std::vector<FinalizeRes> f;
  auto drain = [&]() {
    for (auto& x : r) {
      for (size_t i = 0; i < slots.size(); ++i)
        if (slots[i] == x.slot) {
          out.sse[i] += x.sse;
          out.flags[i] |= x.flags & (RF_DONE | RF_ABORTED);
        }
    }
    r.clear();
  };
  bool more = true;
  while (more) {
    more = false;
    for (size_t i = 0; i < bodies.size(); ++i) {
      if (pos[i] >= bodies[i].size()) continue;
      size_t n = split ? 1 + (size_t)R(40) : bodies[i].size();
      n = std::min(n, bodies[i].size() - pos[i]);
      eng.feed(slots[i], bodies[i].substr(pos[i], n));
      pos[i] += n;
      more = true;
    }
    if (!split || R(2)) {
      eng.tick(1700000000, r, f);
      drain();
    }
  }
  for (int s : slots) eng.finish(s);
  for (int k = 0; k < 8 && eng.has_work(); ++k) {
    eng.tick(1700000000, r, f);
    drain();
  }
  std::vector<int> good;
  for (size_t i = 0; i < slots.size(); ++i)
    if (!(out.flags[i] & RF_ABORTED)) good.push_back(slots[i]);
  int a = eng.submit_finalize(good, true, false, "\n--\n", 1700000000);
  int b = eng.submit_finalize(good, true, true, "", 1700000000);
  for (int k = 0; k < 4 && eng.has_work(); ++k) eng.tick(1700000000, r, f);
  for (auto& x : f) {
    if (x.id == a) out.fin_event = x.event;
    if (x.id == b) out.fin_texts = x.texts;
  }
  for (int s : slots) out.text.push_back(eng.text(s));
  return out;
}

bool same(const Run& x, const Run& y) {
  return x.sse == y.sse && x.flags == y.flags && x.text == y.text && x.fin_event == y.fin_event &&
         x.fin_texts == y.fin_texts;
}

// A random string over the alphabet of the tag grammar (and a little beyond it), or one of the
// shapes a recursive parser can trip over.
std::string rand_tag() {
  static const char* kFixed[] = {"(", "a|", "(?", "a(?", "(a", "a)", "((a)", "a(b|", "a??", "a?*", "|", "()", "(?:)", "a(|)b",
                                 "[", "a[", "a[^", "a[]", "a\\", "?", "a(?:b|c)?(d|e)?(f|g)?(h|i)?(j|k)?"};
  switch (R(8)) {
    case 0: return kFixed[R(sizeof(kFixed) / sizeof(kFixed[0]))];
    case 1: return std::string((size_t)(1 + R(100)), '(') + "a" + std::string((size_t)R(101), ')');
    case 2: return "a" + std::string((size_t)R(100), '?');
    default: break;
  }
  static const char* kAtoms[] = {"a", "b", "t", "(", ")", "(?:", "|", "?", ".", "[0-9]", "[^a]", "[", "]", "\\.", "\\",
                                 "*", "+", "{2}", "é", "思", "<", ">", "/", "^", "$", " ", "X",
                                 "{", "}", ",", "0", "1", "2", "6", "9", "\\d", "\\w", "\\s", "\\D", "{1,2}", "{,3}",
                                 "{2,}", "+", "*", "\\d+", "[a-c]*"};
  std::string t;
  const int n = 1 + R(R(4) == 0 ? 70 : 14);
  for (int i = 0; i < n; ++i) t += kAtoms[R(sizeof(kAtoms) / sizeof(kAtoms[0]))];
  return t;
}

// make_tags over malformed tags: accepted or refused with std::invalid_argument, nothing else.
// An accepted set runs one small stream, so its tables are walked too.
bool malformed_tags_hold() {
  std::vector<std::string> tags;
  const int n = 1 + R(3);
  for (int i = 0; i < n; ++i) tags.push_back(rand_tag());
  const bool unicode = R(2), mixed = R(2), variants = R(4) != 0, extended = R(3) != 0, repeat = R(2) != 0, runs = R(2) != 0;
  try {
    const Tags t = make_tags(tags, true, unicode, mixed, variants, extended, repeat, runs);
    const auto rows = tagset_rows(tags, true, unicode, mixed, variants, extended, repeat, runs);
    if ((int)rows.size() != t.ts.n || t.ts.n > kMaxTags) return false;
    std::string text = "<" + tags[0] + "></" + tags[0] + "><";
    for (const auto& r : rows) text += "<" + r.first + ">x</" + r.first + ">";
    FilterState fs;
    std::string out;
    filter_feed(t, fs, (const uint8_t*)text.data(), text.size(), out);
    (void)strip_final(t, (const uint8_t*)text.data(), text.size());
  } catch (const std::invalid_argument&) {
  }
  return true;
}

std::string rand_json(int depth = 0) {
  int k = R(depth > 3 ? 5 : 8);
  switch (k) {
    case 0: return "null";
    case 1: return R(2) ? "true" : "false";
    case 2: {
      char b[64];
      snprintf(b, sizeof(b), "%.17g", std::ldexp((double)(int64_t)rng() / 9.2e18, R(600) - 300));
      return b;
    }
    case 3: return std::to_string((int64_t)rng() >> R(63));
    case 4: return "\"" + rand_content() + "\"";
    case 5: case 6: {
      std::string s = "[";
      int n = R(4);
      for (int i = 0; i < n; ++i) s += (i ? ", " : "") + rand_json(depth + 1);
      return s + "]";
    }
    default: {
      std::string s = "{";
      int n = R(4);
      for (int i = 0; i < n; ++i) s += (i ? ", \"k" : "\"k") + std::to_string(R(5)) + "\": " + rand_json(depth + 1);
      return s + "}";
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  int iters = argc > 1 ? atoi(argv[1]) : 300;
  rng.seed(argc > 2 ? strtoull(argv[2], nullptr, 10) : 12345);
  const std::vector<std::string> default_tags = {"think", "reason", "reasoning", "thought"};
  int fails = 0;
  for (int it = 0; it < iters; ++it) {
    // every other iteration: one of the class tag sets
    // (then the sets with unbounded repetition once more, with `runs`)
    const int pick = (it / 2) % (kClassSetCount + repeat_sets());
    const bool runs = it % 2 && pick >= kClassSetCount;
    g_class = it % 2 ? &kClassSets[runs ? repeat_set(pick - kClassSetCount) : pick] : nullptr;
    const Tags tags = make_tags(g_class ? g_class->tags : default_tags,
                                g_class != nullptr && (!g_class->unicode || g_class->mixed),
                                g_class != nullptr && g_class->unicode, g_class != nullptr && g_class->mixed,
                                g_class != nullptr && g_class->variants, g_class != nullptr && g_class->extended,
                                g_class != nullptr && g_class->repeat, runs);
    int ns = 1 + R(4);
    std::vector<std::string> bodies;
    std::vector<bool> filt;
    for (int s = 0; s < ns; ++s) {
      std::string b;
      int ne = R(10);
      for (int e = 0; e < ne; ++e) b += rand_event();
      if (R(4) == 0 && !b.empty()) b.resize(b.size() - (size_t)R((int)std::min<size_t>(b.size(), 5)));
      bodies.push_back(b);
      filt.push_back(R(5) != 0);
    }
    Run whole = run_engine(tags, bodies, filt, false);
    Run split = run_engine(tags, bodies, filt, true);
    if (!same(whole, split)) {
      if (++fails <= 3) fprintf(stderr, "streaming invariance violated (iteration %d)\n", it);
    }
    if (!malformed_tags_hold()) {
      if (++fails <= 3) fprintf(stderr, "malformed tags: rows and tables disagree (iteration %d)\n", it);
    }
    if (runs) {
      const std::string text = rand_content() + rand_content() + rand_content();
      if (!device_rule_holds(tags, text) && ++fails <= 3)
        fprintf(stderr, "device candidate rule differs from the exact walk (iteration %d): %s\n", it, text.c_str());
      // the host engines' bytes do not depend on `runs`
      const Tags plain = make_tags(g_class->tags, !g_class->unicode || g_class->mixed, g_class->unicode, g_class->mixed,
                                   g_class->variants, g_class->extended, g_class->repeat);
      if (!same(whole, run_engine(plain, bodies, filt, false)) && ++fails <= 3)
        fprintf(stderr, "runs changed the host engine's output (iteration %d)\n", it);
    }
    // strip_final: stripping a stripped text (no tags left in it) only re-strips whitespace
    std::string t = rand_content() + rand_content();
    std::string s1 = strip_final(tags, (const uint8_t*)t.data(), t.size());
    std::string s2 = strip_final(tags, (const uint8_t*)s1.data(), s1.size());
    (void)s2;
    // JSON DOM round trip
    std::string js = rand_json();
    JVal v1, v2;
    std::string err;
    if (json_parse(js.data(), js.size(), v1, &err)) {
      std::string d1 = json_dumps(v1);
      if (!json_parse(d1.data(), d1.size(), v2, &err) || json_dumps(v2) != d1) {
        if (++fails <= 3) fprintf(stderr, "json round trip failed: %s\n", js.c_str());
      }
    }
    double x = std::ldexp((double)(int64_t)rng(), R(200) - 100);
    std::string rep = py_float_repr(x);
    std::string esc;
    escape_append((const uint8_t*)t.data(), t.size(), esc);
    (void)rep;
  }
  printf("{\"iterations\": %d, \"failures\": %d}\n", iters, fails);
  return fails ? 1 : 0;
}
