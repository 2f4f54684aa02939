"""Boundary inputs for the tick kernel (S0-S6) and the finalize items (K3-K5): pure Python
generators, no engine.

Every generator takes the limits dict of the native module (``kernel_limits()``) and places
its inputs on, just below and just above one of them, so a retuned limit moves its sweep.
A :class:`Case` is one engine run (``engine_harness.run_case``): all offsets of a sweep are
streams of that one run — many workgroups in a few launches.  Every input is a valid
upstream byte stream; the ``+1`` cases that hand a stream to the host path by design say so in
``escalations``.

``families(L)`` returns {family letter: [Case, ...]}:

  A  tile load and framing        D  S5 / S6 output
  B  S3 templates                 E  K3 / K4 / K5 finalize
  C  S4 filter
"""
from __future__ import annotations

import json
from typing import Dict, List, NamedTuple, Optional, Sequence

import engine_harness as H


class Case(NamedTuple):
    name: str
    tags: Sequence[str]
    streams: List[List[bytes]]           # chunk lists, one per stream
    filt: List[bool]
    emit: List[bool]
    indices: Optional[List[int]] = None  # backend index per stream (default i % 7)
    strips: Sequence[bool] = (True,)     # strip_final values to run the case with
    joiner: str = "\n---\n"
    kw: Optional[dict] = None            # engine keyword arguments (tile_bytes, content_cap)
    eof_with_last: Optional[List[bool]] = None
    groups: Optional[List[List[int]]] = None  # finalize requests (default: one over all streams)
    every_round: bool = False            # tick after every round of feeds (fixed schedule)
    escalations: int = 0                 # streams the HIP engine hands to the host path by design
    requeues: Optional[int] = None       # tiles cut at MAX_EV events (None: not pinned)


DONE = b"data: [DONE]\n\n"

# thresholds the kernel writes as plain numbers (kernel_limits() has the named ones)
S2_WAVE_FRAME = 4096   # s2_wave: first frame of at most this many bytes at an 8-aligned start
WAVE_EVENTS = 64       # S3 / S4 / S6: up to one wave's lanes of events (deltas) in a tile
S4_WAVE_ZN = 2048      # s4_wave / s6_wave: at most this many decoded (kept) bytes
S4_WAVE_CAND = 63      # s4_wave gives up above it
SMALL_TILE = 1024      # the smallest tile an engine takes


def around(x: int, d: int = 2) -> List[int]:
    return list(range(x - d, x + d + 1))


def jstr(text: str, ascii_only: bool = True) -> bytes:
    """A JSON string literal; lone surrogates only exist in the escaped form."""
    if not ascii_only:
        try:
            return json.dumps(text, ensure_ascii=False).encode()
        except UnicodeEncodeError:
            pass
    return json.dumps(text).encode()


def cev(text: str, ascii_only: bool = True) -> bytes:
    """The shortest upstream content event."""
    return b'data: {"choices":[{"delta":{"content":' + jstr(text, ascii_only) + b"}}]}\n\n"


CEV0 = len(cev(""))


def cev_len(n: int, fill: str = "x") -> bytes:
    """A content event of exactly n bytes (separator included) stretched with filler."""
    assert n >= CEV0, n
    return cev(fill * (n - CEV0))


def text_stream(text: str, piece: int = 3000, ascii_only: bool = True) -> bytes:
    """A text of any length as content events of at most `piece` characters each."""
    return b"".join(cev(text[i:i + piece], ascii_only) for i in range(0, len(text), piece)) or b""


def _case(name, tags, streams, filt=True, emit=True, **kw) -> Case:
    n = len(streams)
    return Case(name, list(tags), [list(s) for s in streams], [filt] * n if isinstance(filt, bool) else list(filt),
                [emit] * n if isinstance(emit, bool) else list(emit), **kw)


# moved here from test_gpu_engine.py: the OpenAI-shaped events of the hole-template tests
def _oai_event(id_, created, model, delta, finish=b"null", compact=False, extra=b""):
    sep = b"," if compact else b", "
    col = b":" if compact else b": "
    obj = (b"{" + b'"id"' + col + b'"' + id_ + b'"' + sep + b'"object"' + col + b'"chat.completion.chunk"' + sep +
           b'"created"' + col + created + sep + b'"model"' + col + b'"' + model + b'"' + sep + extra + b'"choices"' + col +
           b'[{"index"' + col + b"0" + sep + b'"delta"' + col + delta + sep + b'"logprobs"' + col + b"null" + sep +
           b'"finish_reason"' + col + finish + b"}]}")
    return b"data: " + obj + b"\n\n"


# hole contents: valid and invalid string bodies / numbers, type changes
HOLE_STR = [b"abc", b"", b'q\\"x', b"\\u00e9\\ud83d\\ude00", b"\xc3\xa9 ok", b"bad\xff", b"tail\\\\", b"a\\", b"x\x01y",
            b"\\uZZZZ", b"<think>", b"</think>", b"e\\nf", b"\\/", b"\xe4\xb8\xad" * 20, b"q" * 120]
HOLE_NUM = [b"1700000000", b"0", b"-1", b"01", b"1.5e3", b"-", b"1e400", b"123456789012345678901234567890123456",
            b"2.", b"-0", b"1E+2", b"true", b"null", b'"1700000000"']


# ------------------------------------------------------------------------------------------
# A. tile load and framing
# ------------------------------------------------------------------------------------------
def _feed_of(n: int) -> bytes:
    """n bytes of complete events: three small ones, one stretched to hit n exactly."""
    head = cev("ab") + cev("<") + cev("c d")
    return head + cev_len(n - len(head))


def family_a(L) -> List[Case]:
    spec, tile, max_ev = L["kSpecTile"], L["TILE_MAX"], L["MAX_EV"]
    cases = []
    # S0: the speculative first load ends at kSpecTile, the second at TILE_MAX; every length of
    # the last 16-byte vector
    ns = list(range(spec - 17, spec + 18)) + list(range(tile - 17, tile + 2))
    cases.append(_case("A_feed_len", ["think"], [[_feed_of(n)] for n in ns]))
    # the "\n\n" that ends an event at tile end -2, -1 (split between two submissions), 0, +1;
    # small events first, so the first tile makes progress (the smallest tile runs these
    # separator positions only: the feed-length sweep above needs events longer than it holds)
    for tb, kw in ((SMALL_TILE, {"tile_bytes": SMALL_TILE}), (tile, None)):
        streams = []
        for p in range(tb - 2, tb + 2):
            head = cev("a<think>b</think>c") * 6
            streams.append([head + cev_len(p + 2 - len(head)) + cev("</think>z") + cev("tail") + DONE])
        cases.append(_case(f"A_sep_at_tile_end_{tb}", ["think"], streams, kw=kw))
    # S2: the one-wave framing takes a tile whose bytes after the start (in_len - start: the
    # whole first feed but its leading whitespace, which is stripped at stream start and moves
    # the start) are at most 4096, at an 8-aligned start.  The first chunk is exactly that
    # long; the rest of the stream comes a tick later
    streams = []
    for lead in (b"", b" ", b"   ", b" " * 8):
        for n in around(S2_WAVE_FRAME):
            head = cev("a") + cev("<think>")
            streams.append([lead + head + cev_len(n - len(head)), cev("</think>b") + DONE])
    cases.append(_case("A_first_frame", ["think"], streams, every_round=True))
    # S3: one wave handles up to 64 events
    cases.append(_case("A_events_64", ["think"], [[cev("a") * n + DONE] for n in around(WAVE_EVENTS)]))
    # MAX_EV events in one tile: mostly 5-9-byte skip events, content events / [DONE] as event
    # number MAX_EV-1, MAX_EV, MAX_EV+1 (1-based), with the end of input in the same tick and
    # a tick later
    skips = [b": k\n\n", b"data:{}\n\n"]

    def many(total, special):  # special: {1-based event number: bytes}
        return b"".join(special.get(k, skips[k & 1]) for k in range(1, total + 1))

    streams, eof = [], []
    marks = (max_ev - 1, max_ev, max_ev + 1)
    for with_eof in (True, False):
        for total in range(max_ev - 1, max_ev + 3):
            streams.append([many(total, {k: cev("e%d." % k) for k in marks})])
            eof.append(with_eof)
        for k in marks:
            streams.append([many(max_ev + 2, {k: DONE, k + 1: cev("after done")})])
            eof.append(with_eof)
        # exactly MAX_EV separators, then an unterminated content event at the end of input
        streams.append([many(max_ev, {1: cev("first")}) + cev("unterminated")[:-2]])
        eof.append(with_eof)
    # tiles cut at MAX_EV events: per half, the totals MAX_EV+1 and +2, the three [DONE] streams,
    # and (only with the end of input in the same tick) the unterminated event after MAX_EV
    cases.append(_case("A_max_ev", ["think"], streams, eof_with_last=eof, every_round=True, requeues=2 * 5 + 1))
    return cases


# ------------------------------------------------------------------------------------------
# B. S3 templates
# ------------------------------------------------------------------------------------------
def tpl_stream(pre_len: int, suf_len: int) -> List[bytes]:
    """Events whose bytes before the content string body are pre_len long and whose bytes from
    the closing quote on are suf_len long (separator excluded): 3 warm events, 4 that differ
    in content only, one that differs in the byte before the opening quote, one that differs in
    the byte after the closing quote, 2 more of the first shape — one event per chunk."""
    p0, p1 = b'data: {"id": "', b'", "choices": [{"delta": {"content": "'
    s0, s1 = b'" }}], "pad": "', b'"}'
    pre = p0 + b"i" * (pre_len - len(p0) - len(p1)) + p1
    suf = s0 + b"p" * (suf_len - len(s0) - len(s1)) + s1
    assert len(pre) == pre_len and len(suf) == suf_len, (pre_len, suf_len)
    pre_v = pre[:-2] + b'\t"'
    suf_v = b'"\t' + suf[2:]
    evs = [pre + b"warm" + suf] * 3
    evs += [pre + c + suf for c in (b"one", b"", b"a\\nb <think>", b"x" * 70)]
    evs += [pre_v + b"pv" + suf, pre + b"</think>sv" + suf_v, pre + b"back" + suf, pre + b"again" + suf]
    return [e + b"\n\n" for e in evs]


def oai_stream(id_: bytes, model: bytes, extra: bytes = b"", n_content: int = 4) -> List[bytes]:
    """A role event, content events, a finish event and [DONE]: one event per chunk."""
    evs = [_oai_event(id_, b"1700000001", model, b'{"role": "assistant", "content": ""}', extra=extra)]
    for k in range(n_content):
        evs.append(_oai_event(id_, b"17000000%02d" % k, model, b'{"content": "tok%d <"}' % k, extra=extra))
    evs.append(_oai_event(id_, b"1700000009", model, b"{}", finish=b'"stop"', extra=extra))
    return evs + [DONE]


def _oai_content_len(id_, model, extra=b""):
    return len(_oai_event(id_, b"1700000000", model, b'{"content": "tok0 <"}', extra=extra)) - 2


def tpl_pre_cases(L):
    return [(n, _case(f"B_tpl_pre_{n}", ["think"], [tpl_stream(n, 40)], every_round=True)) for n in around(L["TPL_PRE_MAX"])]


def tpl_suf_cases(L):
    return [(n, _case(f"B_tpl_suf_{n}", ["think"], [tpl_stream(120, n)], every_round=True)) for n in around(L["TPL_SUF_MAX"])]


def hole_len_cases(L):
    """OpenAI-shaped events whose content events are n bytes long, n around kHoleTplBytes (the
    model name is padded: the content string starts past TPL_PRE_MAX, so no per-stream
    template takes these events)."""
    out = []
    base = _oai_content_len(b"chatcmpl-1", b"")
    for n in around(L["kHoleTplBytes"]):
        model = b"m" * (n - base)
        assert _oai_content_len(b"chatcmpl-1", model) == n
        # two streams, one after the other in one run: the second one's events find the hole
        # templates the first one published
        out.append((n, _case(f"B_hole_len_{n}", ["think"],
                             [oai_stream(b"chatcmpl-1", model), [b""] * 8 + oai_stream(b"chatcmpl-2", model)],
                             indices=[0, 0], every_round=True)))
    return out


def holes_event(digit: int, k: int, text: bytes) -> bytes:
    """A short content event with k one-digit numbers before choices: k + 1 holes (the numbers
    and the content string) in 24 + 2k JSON tokens — '{', "n" (2), ':', '[', k numbers and
    k - 1 commas, ']', ',', then 17 for the rest — so it stays within the 64 tokens up to
    which a parsed event is published as a hole template."""
    return (b'data: {"n":[' + b",".join([b"%d" % digit] * k) + b'],"choices":[{"delta":{"content":"' + text + b'"}}]}\n\n')


def hole_count_cases(L):
    """Events with nh holes, nh around kHoleMax.  The digits differ from event to event, so the
    stream's own prefix template never matches and only a hole template can spare the parse."""
    out = []
    for nh in around(L["kHoleMax"]):
        k = nh - 1
        assert 24 + 2 * k <= 64
        streams = [[holes_event(1 + (e + 4 * j) % 9, k, b"tok%d" % e) for e in range(4)] + [DONE] for j in range(2)]
        streams[1] = [b""] * 6 + streams[1]  # after the first stream: its templates exist
        out.append((nh, _case(f"B_hole_count_{nh}", ["think"], streams, indices=[0, 0], every_round=True)))
    return out


def backend_index_cases(L):
    """Two OpenAI-shaped streams, one after the other, on a backend index with (0,
    kBackendTpl - 1) and without (kBackendTpl, + 1) a template table entry."""
    nb = L["kBackendTpl"]
    return [(i, _case(f"B_backend_index_{i}", ["think"],
                      [oai_stream(b"chatcmpl-1", b"mock"), [b""] * 8 + oai_stream(b"chatcmpl-2", b"mock")],
                      indices=[i, i], every_round=True)) for i in (0, nb - 1, nb, nb + 1)]


def s3a_len_cases(L):
    """OpenAI-shaped streams whose content events are n bytes long, n around the 256 bytes that
    the S3a prepass (half a wave per event, a hole template's word masks) covers: longer
    events are left to the S3 loop."""
    out = []
    base = _oai_content_len(b"chatcmpl-1", b"")
    for n in around(L["kHoleWmaskBytes"]):
        model = b"m" * (n - base)
        assert _oai_content_len(b"chatcmpl-1", model) == n
        out.append((n, _case(f"B_s3a_len_{n}", ["think"],
                             [oai_stream(b"chatcmpl-1", model), [b""] * 8 + oai_stream(b"chatcmpl-2", model)],
                             indices=[0, 0], every_round=True)))
    return out


def family_b(L) -> List[Case]:
    cases = [c for _, c in tpl_pre_cases(L) + tpl_suf_cases(L) + hole_len_cases(L) + hole_count_cases(L) +
             backend_index_cases(L) + s3a_len_cases(L)]
    # the content hole starting at byte 250 ... 262 of the event (the S3 loop's hole match: the
    # prepass takes no event this long, see s3a_len_cases)
    w = L["kHoleWmaskBytes"]
    streams = []
    base = _oai_content_len(b"", b"mock") - len(b'tok0 <"}, "logprobs": null, "finish_reason": null}]}')
    for o in range(w - 6, w + 7):
        streams.append(oai_stream(b"c" * (o - base), b"mock"))
        ev = streams[-1][1]
        assert ev.index(b"tok0") == o, (o, ev.index(b"tok0"))
    streams += [[b""] * 8 + s for s in streams]
    cases.append(_case("B_hole_offset", ["think"], streams, indices=[i % 13 for i in range(13)] * 2, every_round=True))
    # JSON token counts around TOK_CAP: an "n": [1,1,...] member of m numbers before choices is
    # 24 + 2m tokens (holes_event's count), TOK_CAP at m = (TOK_CAP - 24) / 2
    m0 = (L["TOK_CAP"] - 24) // 2
    streams = [[b'data: {"n": [' + b",".join([b"1"] * m) + b'], "choices": [{"delta": {"content": "t%d"}}]}\n\n' % m + DONE]
               for m in around(m0, 3)]
    cases.append(_case("B_tok_cap", ["think"], streams))
    return cases


# ------------------------------------------------------------------------------------------
# C. S4 filter
# ------------------------------------------------------------------------------------------
def _name(n: int, step: int) -> str:
    """A tag of n distinct-looking letters (a shifted or skipped byte shows)."""
    return "".join(chr(97 + (i * step + n) % 26) for i in range(n))


def cand_text(c: int, where: str) -> str:
    """c '<' candidates: plain '<.' ones and, from 2 on, one real <t>hidden</t> pair as the
    first, the middle or the last two of them."""
    if c < 2:
        return "a" + "<." * c + "z"
    plain = c - 2
    k = {"first": 0, "middle": plain // 2, "last": plain}[where]
    return "a" + "<." * k + "<t>hidden</t>" + "<." * (plain - k) + "z"


def family_c(L) -> List[Case]:
    mc, tail, tl, win = L["MAX_CAND"], L["kMaxTail"], L["kMaxTagLen"], L["kWindow"]
    cases = []
    counts = [0, 1] + around(4) + around(win) + around(2 * win) + around(S4_WAVE_CAND) + [mc - 1, mc]
    streams = [[cev(cand_text(c, wh)) + DONE] for c in counts for wh in ("first", "middle", "last")]
    cases.append(_case("C_cand_counts", ["t"], streams))
    streams = [[cev(cand_text(mc + 1, "middle")) + DONE]]
    cases.append(_case("C_cand_over", ["t"], streams, escalations=1))
    # the two routes into the filter: Zn around 2048 (one delta), ndelta around 64, both
    streams = [[cev("a<t>h</t>" + "x" * (n - 11) + "<.") + DONE] for n in around(S4_WAVE_ZN)]
    streams += [[cev("a<t>h</t>b<") * n + DONE] for n in around(WAVE_EVENTS)]
    streams += [[cev("a<t>h</t>b<") * n + cev("x" * (S4_WAVE_ZN + d - 11 * n)) + DONE] for n in (WAVE_EVENTS - 1, WAVE_EVENTS) for d in (-1, 0, 1)]
    # ndelta around 64 with few candidates: the one-wave filter decides by ndelta alone; at 64
    # deltas its holdback tail is cut on lane 0 — with a tag prefix at the end of Z outside a
    # block (held) and inside one (carried)
    for n in around(WAVE_EVENTS):
        texts = ["ab"] * n
        for i in (0, n // 3, n // 2, n - 2):
            texts[i] = "a<t>h</t>b"
        streams.append([b"".join(cev(x) for x in texts) + DONE])
        streams.append([b"".join(cev(x) for x in texts[:-1]) + cev("x<t"), cev(">hid</t>y") + DONE])
        streams.append([b"".join(cev(x) for x in texts[:-1]) + cev("<t>h</"), cev("t>y") + DONE])
    cases.append(_case("C_routes", ["t"], streams, every_round=True))
    # 8 / 9 / 16 tags: one and two 16-pattern column blocks
    for nt in (8, 9, L["kMaxTags"]):
        tags = ["tag%c" % (97 + i) for i in range(nt)]
        streams = []
        for t in tags:
            txt = f"a<{t}>hid</{t}>b<{t.upper()}>h</{t.title()}>c<{t}x>d</{t}>e<{t[:-1]}>f"
            streams.append([cev(txt) + DONE])
        streams.append([b"".join(cev(f"<{t}>") for t in tags) + cev("in") + b"".join(cev(f"</{t}>") for t in tags) + cev("out") + DONE])
        cases.append(_case(f"C_tags_{nt}", tags, streams))
    # patterns of 15, 16, 17 bytes around the 16-byte match window, and the longest tag; near
    # misses that differ only in the byte at pattern offset 15, 16, 17
    tags = [_name(k, 7) for k in range(win - 4, win)] + [_name(tl, 1)]
    streams = []
    for t in tags:
        op, cl = f"<{t}>", f"</{t}>"
        streams.append([cev(f"a{op}hid{cl}b{op.upper()}h{cl.upper()}c") + DONE])
        for off in (win - 1, win, win + 1):
            for pat, txt in ((op, "a%sb" + cl + "c"), (cl, "a" + op + "h%sstill" + cl + "c")):
                if off < len(pat):
                    bad = pat[:off] + "~" + pat[off + 1:]
                    streams.append([cev(txt % bad) + DONE])
    cases.append(_case("C_long_tags", tags, streams))
    # holdback: an open and a close of the longest tag cut after every prefix length, the two
    # parts in events of different ticks; also case-folded, and a prefix that turns out no tag
    t = _name(tl, 3)
    assert len(f"</{t}>") == tail
    streams = []
    for fold in (str, str.upper):
        op, cl = fold(f"<{t}>"), fold(f"</{t}>")
        for k in range(1, tail):
            streams.append([cev("a" + op[:k]), cev(op[k:] + "hid" + cl + "b"), DONE])
            streams.append([cev("a" + f"<{t}>" + "h" + cl[:k]), cev(cl[k:] + "b"), DONE])
    for k in range(1, tail):
        streams.append([cev("a" + f"<{t}>"[:k]), cev("~b"), DONE])
        # no tag prefix from its last byte on: released with its own event, not a tick later
        streams.append([cev("a" + f"<{t}>"[:k] + "~"), cev("b"), DONE])
    cases.append(_case("C_holdback_cuts", [t], streams, every_round=True))
    cases.append(deep_nesting_case(L))
    return cases


WRAP = 1 << 16  # where a 16-bit depth counter is 0 again


def deep_nesting_case(L) -> Case:
    """Think blocks nested past 32768 and 65536 levels, one event of <t> x per_tick per tick
    (under MAX_CAND candidates: the block path), small steps of 60 (the one-wave filter).
    By the reference's counting none of the letters is outside every block."""
    per = L["MAX_CAND"] - 24
    op, cl = "<t>", "</t>"
    big = cev(op * per)
    full, rest = divmod(WRAP, per)
    assert S4_WAVE_CAND < rest <= L["MAX_CAND"]
    issue = ([big] * (WRAP // 2 // per + 1) + [cev("A")] + [big] * (WRAP // 2 // per + 1) + [cev("B"), cev(cl * 10), cev("C"), DONE])
    streams = [
        issue,
        # the block path lands exactly on 65536; the text comes in the next tick / the same event
        [big] * full + [cev(op * rest), cev("A"), cev(cl * 3 + "B"), DONE],
        [big] * full + [cev(op * rest + "A"), cev(cl * 3 + "B"), DONE],
        # the one-wave filter lands on it
        [big] * full + [cev(op * 60)] * ((rest - 1) // 60) + [cev(op * ((rest - 1) % 60 + 1)), cev("A"), cev(cl * 3 + "B"), DONE],
        [big] * full + [cev(op * 60)] * ((rest - 1) // 60) + [cev(op * ((rest - 1) % 60 + 1) + "A<"), cev(cl * 3 + "B"), DONE],
        # past it, then as many closes as a wrapped counter would need to reach 0
        [big] * (full + 1) + [cev(cl * (per - rest) + "D"), cev(cl * 3 + "E<t"), DONE],
        [big] * (full + 1) + [cev(cl * 50)] * ((per - rest) // 50) + [cev(cl * ((per - rest) % 50) + "D"), DONE],
        [cev("visible"), DONE],  # (so the session has a final text)
    ]
    return _case("C_deep_nesting", ["t"], streams, every_round=True)


# ------------------------------------------------------------------------------------------
# D. S5 / S6 output
# ------------------------------------------------------------------------------------------
def family_d(L) -> List[Case]:
    from quorum_amd.ops import reference as ref

    tile = L["TILE_MAX"]
    cases = []
    # content_cap exact fit: the stream one byte over goes to the host path by design
    cap = 256
    streams = [[cev("x" * (n - 100)), cev("y" * 100), DONE] for n in (cap - 1, cap, cap + 1)]
    cases.append(_case("D_content_cap", ["think"], streams, filt=False, kw={"content_cap": cap}, escalations=1,
                       every_round=True))
    # out_cap = 12 x submitted bytes + 1024.  The shortest content event is CEV0 + 1 bytes of
    # input for one envelope plus at most 12 output bytes (a 4-byte character, 12 / 4 bytes of
    # input, is the worst ratio per content byte): the envelope is under 12 x CEV0 bytes (asserted
    # here), so no valid input exceeds the cap and only the nearest approach is run — a full
    # tile of shortest events, each with one control character (6 output bytes for 6 of input)
    # or one 4-byte character (12 for 4)
    evl = len(ref.delta_event(100, H.CREATED, ""))
    assert evl + 12 <= 12 * (CEV0 + 1)
    for name, ch, asc in (("ctl", "\x01", True), ("astral", "\U0001f600", False)):
        e = cev(ch, asc)
        cases.append(_case(f"D_out_cap_near_{name}", ["think"], [[e * (tile // len(e))]], indices=[100]))
    # output windows: a stream emitting just over 1, 2, 3 windows of TILE_MAX bytes in one tick;
    # the length of the first event's content moves every later envelope over the window edges
    for fill, asc, name, nwin in (("a", True, "ascii", (1, 2, 3)), ("é", False, "u00e9", (1,)),
                                  ("\U0001f600", False, "pair", (1,)), ("\n", True, "nl", (1,))):
        evn = len(ref.delta_event(0, H.CREATED, fill))
        for k in nwin:
            n = k * tile // evn + 2
            # (one envelope's length of shifts: each window edge meets every byte of an envelope,
            # every split of an escape sequence among them)
            streams = [[(cev("b" * j) if j else b"") + cev(fill, asc) * n + DONE] for j in range(evn)]
            assert all(len(s[0]) <= tile for s in streams)
            cases.append(_case(f"D_window_{name}_{k}", ["think"], streams, filt=[j & 1 == 0 for j in range(evn)],
                               indices=[0] * evn))
    # S6 sizing on one wave: Wlen around 2048, ndelta around 64, emit on
    streams = [[cev("x" * n) + DONE] for n in around(S4_WAVE_ZN)] + [[cev("ab") * n + DONE] for n in around(WAVE_EVENTS)]
    streams += [[cev("é" * (n // 2), False) + DONE] for n in around(S4_WAVE_ZN, 4)]
    cases.append(_case("D_sizing_wave", ["think"], streams, filt=False))
    # json.dumps escape classes and UTF-8 lengths: the first and last code point of each, raw
    # in the upstream event and escaped
    edges = [0x1f, 0x20, 0x7e, 0x7f, 0x80, 0x7ff, 0x800, 0xd7ff, 0xe000, 0xffff, 0x10000, 0x10ffff]
    streams = [[cev("a" + chr(c) + "b" + chr(c), asc) + DONE] for c in edges for asc in (True, False)]
    cases.append(_case("D_escape_edges", ["think"], streams))
    # clean vs general: identical but for one '"' in the last byte of the last event
    body = cev("plain text") * 20
    cases.append(_case("D_clean_vs_general", ["think"], [[body + cev("last.") + DONE], [body + cev('last"') + DONE]]))
    return cases


# ------------------------------------------------------------------------------------------
# E. K3 / K4 / K5 finalize (unfiltered streams: the tags stay in the texts)
# ------------------------------------------------------------------------------------------
NEIGHBOURS = ["\u200b", "\u2007", "\u180e", "\u0084", "\u001b", "\ufeff", "\u2060"]


def space_chars() -> List[str]:
    return [chr(c) for c in range(0x110000) if chr(c).isspace()]


def _fin(name, tags, texts, **kw) -> Case:
    kw.setdefault("strips", (True, False))
    return _case(name, tags, [[text_stream(t, ascii_only=False)] if t else [] for t in texts], filt=False, emit=False, **kw)


def family_e(L) -> List[Case]:
    win, big, bs, tl = L["FIN_WIN"], L["FIN_BIG"], L["BS"], L["kMaxTagLen"]
    long_tag = _name(tl, 5)
    tags = ["think", long_tag]
    lo, lc = f"<{long_tag}>", f"</{long_tag}>"
    cases = []
    # a token starting at every offset from FIN_WIN-66 to FIN_WIN+1: an open, a close, a 64-byte
    # close, a near miss
    offs = range(win - 66, win + 2)
    fill = "y" * 3
    cases.append(_fin("E_win_open", tags, ["a" * o + "<think>hid</think>" + fill for o in offs]))
    cases.append(_fin("E_win_close", tags, ["<think>" + "h" * (o - 7) + "</think>" + fill for o in offs]))
    cases.append(_fin("E_win_close64", tags, [lo + "h" * (o - len(lo)) + lc + fill for o in offs]))
    cases.append(_fin("E_win_near_miss", tags, ["<think>" + "h" * (o - 7) + "</thinq>i</think>" + fill for o in offs]))
    texts = [
        "a<think>" + "h" * (2 * win) + "</think>b",      # opened in window 0, closed in window 2
        "</think>" + "k" * win + "<think>kept",           # the only close lies in an earlier window
        "</think><think>" + "k" * win + "<think>k</think>z",
    ]
    # the selected close as token 63, 64, 65 (and 127 ... 129) of its window
    texts += ["<think>" + "<think>" * (k - 1) + "</think>z" + "<think>q</think>" for k in around(WAVE_EVENTS) + around(2 * WAVE_EVENTS)]
    cases.append(_fin("E_windows_tokens", tags, texts))
    # kept segments around FIN_BIG; 511, 512, 513 kept segments; the most segments per byte
    texts = ["x" * n + "<t>h</t>" + "y" * n + "<T>h</T>" + "z" * n for n in around(big, 1)]
    texts += ["k<t>h</t>" * (n - 1) + "k" for n in around(bs, 1)]
    texts += ["<t></t>k" * n for n in (1, 8, win // 8, win // 8 + 1)]
    cases.append(_fin("E_segments", ["t"], texts))
    # str.strip(): every white-space code point and its non-space neighbours at the head and
    # tail of a text, next to a removed interval, and as the whole text (which then strips to
    # nothing, between non-empty texts: the joiner count)
    texts = []
    for c in space_chars() + NEIGHBOURS:
        texts += [c + "ab" + c, "a" + c + "<think>h</think>" + c + "b", c + "<think>h</think>" + c, c]
    cases.append(_fin("E_strip_edges", ["think"], texts))
    # (a text cannot end in a truncated white-space lead byte: an event with invalid UTF-8 is
    # skipped whole, and a lone surrogate's three bytes start with 0xED, no white-space lead)
    # K5: per-thread chunks of C = ceil(jl / BS) bytes moved to code-point starts: a 2-, 3-,
    # 4-byte character and a lone surrogate at every offset 0 ... 2C, joined lengths around BS
    # and 2 x BS; every output length mod 16 comes with the 31 consecutive lengths
    for name, ch in (("2", "é"), ("3", "中"), ("4", "\U0001f600"), ("lone", "\ud83d")):
        texts = []
        nb = len(ch.encode("utf-8", "surrogatepass"))
        for jl in list(range(bs - 12, bs + 19)) + list(range(2 * bs - 4, 2 * bs + 7)):
            c = -(-jl // bs)
            texts += ["a" * o + ch + "b" * (jl - o - nb) for o in range(2 * c + 1)]
        cases.append(_fin(f"E_k5_char_{name}", ["think"], texts, groups=[[i] for i in range(len(texts))]))
    # two adjacent lone surrogates from separate events at the chunk edges
    streams = [[cev("a" * o + "\ud83d") + cev("\ude00" + "b" * (2 * bs + 2 - o - 6))] for o in range(9)]
    cases.append(_case("E_k5_surrogate_halves", ["think"], streams, filt=False, emit=False,
                       groups=[[i] for i in range(9)], strips=(True, False)))
    # joiners of 0, 1, 15, 16, 17 bytes, one of them multi-byte
    for j, joiner in enumerate(("", "|", "-" * 15, "=" * 16, "é" * 8 + "|", "\U0001f600\n--\n" + "中" * 2 + "12")):
        assert len(joiner.encode()) in (0, 1, 15, 16, 17)
        cases.append(_fin(f"E_joiner_{j}", ["think"], ["one", " <think>x</think> ", "twoé", "three"], joiner=joiner))
    # 1, 8, 9, 17 texts per request
    texts = ["t%d <think>h</think>é" % i for i in range(35)]
    cases.append(_fin("E_texts_per_request", ["think"], texts,
                      groups=[[0], list(range(1, 9)), list(range(9, 18)), list(range(18, 35))]))
    return cases


def families(L) -> Dict[str, List[Case]]:
    return {"A": family_a(L), "B": family_b(L), "C": family_c(L), "D": family_d(L), "E": family_e(L)}
