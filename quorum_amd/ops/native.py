"""Loader for the native extension ``quorum_amd/_qmx*.so`` (C++ host library + CDNA4 kernels).

The extension is built in-tree by ``python -m quorum_amd.ops.build`` (or
``__graft_entry__.build()``).  On a GPU box a missing extension is an error, never a
silent fallback: :func:`require` raises with the build command.
"""
from __future__ import annotations

import importlib
import os
from typing import Callable, List, Optional, Sequence

_ext = None
_err: Optional[BaseException] = None


def _load():
    global _ext, _err
    if _ext is not None or _err is not None:
        return _ext
    try:
        _ext = importlib.import_module("quorum_amd._qmx")
    except BaseException as exc:  # noqa: BLE001
        _err = exc
    return _ext


def available() -> bool:
    return _load() is not None


def require():
    ext = _load()
    if ext is None:
        raise RuntimeError(
            "quorum_amd native extension is not built (python -m quorum_amd.ops.build): "
            f"{_err!r}")
    return ext


def gpu_available() -> bool:
    """True when the HIP runtime sees a device (does not initialise torch)."""
    if os.environ.get("QMX_FORCE_CPU") == "1":
        return False
    ext = _load()
    if ext is None:
        return False
    try:
        return ext.device_count() > 0
    except Exception:  # noqa: BLE001
        return False


def sent_tags(tags: Sequence[str], classes: bool = False, unicode: bool = False, mixed: bool = False,
              variants: bool = False, extended: bool = False, repeat: bool = False, runs: bool = False) -> List[str]:
    """The tag list as it is sent to the extension, first occurrence only.  Class and non-ASCII
    tags go down as written (lowercasing would turn "[Z-a]" into another pattern; the C++ parser
    folds non-ASCII tags through its pair table), plain tags through ``str.lower()``, which is
    more than ASCII lowercasing: "THIN\u212a" (Kelvin sign) is "think" and runs; as written it would not.
    (``mixed`` needs both other keys, ``variants`` needs ``classes``, ``extended`` needs ``variants``
    and ``repeat`` needs ``extended``, so they change nothing here; neither does ``runs``, which changes only
    what the GPU decides.)"""
    return list(dict.fromkeys(t if classes or unicode or mixed else t.lower() for t in tags))


def strip_fn(tags: Sequence[str], classes: bool = False, unicode: bool = False,
             mixed: bool = False, variants: bool = False, extended: bool = False, repeat: bool = False, runs: bool = False) -> Callable[[str, bool], str]:
    ext = require()
    stripper = ext.Stripper(sent_tags(tags, classes, unicode, mixed), classes=bool(classes), unicode=bool(unicode),
                            mixed=bool(mixed), variants=bool(variants), extended=bool(extended), repeat=bool(repeat), runs=bool(runs))

    def _strip(text, on):
        if not on:
            return text
        if not isinstance(text, str):
            raise TypeError(f"expected string or bytes-like object, got '{type(text).__name__}'")
        return stripper.strip(text.encode("utf-8", "surrogatepass")).decode("utf-8", "surrogatepass")

    return _strip


def tagset_rows(tags: Sequence[str], classes: bool = False, unicode: bool = False, mixed: bool = False,
                variants: bool = False, extended: bool = False, repeat: bool = False, runs: bool = False) -> List[tuple]:
    """The rows of the tag set the extension builds from ``tags``: ``(row text, index of its tag)``
    in matching order.  A variable-width tag (``variants``) has one row per fixed-width expansion
    in the regex's priority order ("think(ing)?": "thinking", "think"); every other tag has one.
    With ``repeat`` an unbounded quantifier has ``kRepeatRows`` (4) rows beyond its minimum count,
    and the longest is open-ended: its last copy is written with a ``+`` after it and stands for
    "this element, once or more" ("step\\d+": "step\\d\\d\\d\\d+", "step\\d\\d\\d", "step\\d\\d", "step\\d")."""
    return [(str(r), int(i)) for r, i in require().tagset_rows([str(t) for t in tags], bool(classes), bool(unicode),
                                                               bool(mixed), bool(variants), bool(extended), bool(repeat), bool(runs))]


def tagset_ok(tags: Sequence[str], classes: bool = False, unicode: bool = False, mixed: bool = False,
              variants: bool = False, extended: bool = False, repeat: bool = False, runs: bool = False) -> bool:
    """Does the extension run this tag list natively (``make_tags`` is the one definition)?"""
    return bool(require().tagset_ok([str(t) for t in tags], bool(classes), bool(unicode), bool(mixed),
                                    bool(variants), bool(extended), bool(repeat), bool(runs)))


def tagset_kind(tags: Sequence[str], classes: bool = False, unicode: bool = False, mixed: bool = False,
                variants: bool = False, extended: bool = False, repeat: bool = False, runs: bool = False) -> str:
    """"literal", "class", "pair" or "mixed": the kind of the tag set this list makes."""
    return str(require().tagset_kind([str(t) for t in tags], bool(classes), bool(unicode), bool(mixed),
                                     bool(variants), bool(extended), bool(repeat), bool(runs)))


def class_suspects(tags: Sequence[str], text: bytes, strip: bool = False, unicode: bool = False,
                   mixed: bool = False, variants: bool = False, extended: bool = False, repeat: bool = False, runs: bool = False) -> int:
    """Candidates '<' of ``text`` the GPU kernels would hand to the host path (``runs``: by the rule of
    ``runtime.native_run_tags``, which walks a run of ASCII copies past an open-ended row)."""
    return int(require().class_suspects([str(t) for t in tags], bytes(text), bool(strip), bool(unicode),
                                        bool(mixed), bool(variants), bool(extended), bool(repeat), bool(runs)))


def class_candidates(tags: Sequence[str], text: bytes, strip: bool = False, unicode: bool = False,
                     mixed: bool = False, variants: bool = False, extended: bool = False, repeat: bool = False,
                     runs: bool = False) -> List[tuple]:
    """What the GPU kernels decide at every '<' of ``text``, computed on the host by the kernels' own
    candidate rule: ``(position, token, length)`` with token ``+(row + 1)`` an open, ``-(row + 1)`` a
    close, ``0`` no tag here and ``None`` a suspect candidate, which the host path decides."""
    return [tuple(c) for c in require().class_candidates([str(t) for t in tags], bytes(text), bool(strip), bool(unicode),
                                                         bool(mixed), bool(variants), bool(extended), bool(repeat), bool(runs))]


def class_rule_sweep(tags: Sequence[str], alphabet: bytes, max_len: int, strip: bool = False, unicode: bool = False,
                     mixed: bool = False, variants: bool = False, extended: bool = False, repeat: bool = False,
                     runs: bool = False) -> dict:
    """``class_candidates`` against ``class_matches`` at every '<' of ``"<s>x</s>"`` for every string ``s`` of
    at most ``max_len`` bytes of ``alphabet``, enumerated in the extension: the counts ``texts``,
    ``candidates``, ``suspects``, ``matches``, ``beyond_rows`` (matches longer than their row),
    ``mismatched`` and the first few ``mismatches``."""
    return dict(require().class_rule_sweep([str(t) for t in tags], bytes(alphabet), int(max_len), bool(strip), bool(unicode),
                                           bool(mixed), bool(variants), bool(extended), bool(repeat), bool(runs)))


def class_matches(tags: Sequence[str], text: bytes, strip: bool = False, unicode: bool = False,
                  mixed: bool = False, variants: bool = False, extended: bool = False, repeat: bool = False,
                  runs: bool = False) -> List[tuple]:
    """The exact host walk's ``(position, token, length)`` at every '<' of ``text`` (token 0: none)."""
    return [tuple(c) for c in require().class_matches([str(t) for t in tags], bytes(text), bool(strip), bool(unicode),
                                                      bool(mixed), bool(variants), bool(extended), bool(repeat), bool(runs))]


def make_grid(tags: Sequence[str], device: int, doors: int, wg_per_door: int = 8, idle_ms: int = 50,
              classes: bool = False, unicode: bool = False, mixed: bool = False, variants: bool = False, extended: bool = False,
              repeat: bool = False, runs: bool = False):
    """A multi-door loop-tick grid (``HipGrid``) of the kind this tag set's engines need: the
    class kernel for a class tag set (``classes`` on and a '.' or bracket class in a tag), for
    a pair tag set (``unicode`` on and a cased non-ASCII character in a tag) and for a mixed tag
    set (``mixed`` on with both, class elements and non-ASCII literals in one set) and for a set
    with a variable-width tag (``variants`` on with ``classes``: '?', '|', groups; ``extended`` on
    with ``variants``: shorthands and counted repetition; ``repeat`` on with ``extended``: '+', '*'
    and "{m,}" after one element; ``runs`` with ``repeat`` changes no kind), the literal
    kernel otherwise.  Every ``NativeEngine`` given the grid must use the same tags."""
    ext = require()
    cls = bool(classes or unicode) and ext.tagset_has_classes(list(tags), bool(classes), bool(unicode), bool(mixed),
                                                                bool(variants), bool(extended), bool(repeat), bool(runs))
    return ext.HipGrid(device, doors, wg_per_door, idle_ms, classes=cls)


class NativeEngine:
    """Python face of the C++ engines (``cpu`` = host library, ``hip`` = GPU tick kernels)."""

    def __init__(self, kind: str, tags: Sequence[str], device: Optional[int] = None,
                 tile_bytes: int = 16384, max_slots: int = 8192, content_cap: int = 1 << 20, lanes: int = 1,
                 grid=None, door: int = -1, ndoors: int = 1, classes: bool = False, unicode: bool = False,
                 mixed: bool = False, variants: bool = False, extended: bool = False, repeat: bool = False, runs: bool = False):
        ext = require()
        self.kind = kind
        self.name = kind
        self.tags: List[str] = list(tags)
        self.classes = bool(classes)
        self.unicode = bool(unicode)
        self.mixed = bool(mixed)
        self.variants = bool(variants)
        self.extended = bool(extended)
        self.repeat = bool(repeat)
        self.runs = bool(runs)
        low = sent_tags(tags, classes, unicode, mixed)
        if kind == "hip":
            if ext.device_count() <= 0:
                raise RuntimeError("engine 'hip' requested but no GPU is visible")
            if device is None:
                device = int(os.environ.get("LOCAL_RANK", "0")) % max(ext.device_count(), 1)
            # grid: a HipGrid (loop ticks) — this engine posts its ticks into door `door` of it.
            # A class tag set needs a grid made with classes=True (make_grid picks the kind)
            self._e = ext.HipEngine(low, device, tile_bytes, max_slots, content_cap, lanes, grid, door, ndoors,
                                     classes=self.classes, unicode=self.unicode, mixed=self.mixed,
                                     variants=self.variants, extended=self.extended, repeat=self.repeat,
                                     runs=self.runs)
            self.offload = True
        else:
            self._e = ext.CpuEngine(low, classes=self.classes, unicode=self.unicode, mixed=self.mixed,
                                     variants=self.variants, extended=self.extended, repeat=self.repeat,
                                     runs=self.runs)
            self.offload = False
        self.open = self._e.open
        self.feed = self._e.feed
        self.finish = self._e.finish
        self.release = self._e.release
        self.has_work = self._e.has_work

    def submit_finalize(self, req) -> int:
        return self._e.submit_finalize(list(req.slots), bool(req.strip), req.kind == "texts",
                                       req.joiner.encode("utf-8", "surrogatepass"), int(req.created))

    def tick(self, created: int):
        results, fres = self._e.tick(int(created))
        out = []
        for fid, kind, payload in fres:
            if kind == 0:
                out.append((fid, None))
            elif kind == 1:
                out.append((fid, payload))
            else:
                out.append((fid, [p.decode("utf-8", "surrogatepass") for p in payload]))
        return results, out

    def text(self, slot: int) -> str:
        return self._e.text(slot).decode("utf-8", "surrogatepass")

    def stats(self) -> dict:
        return dict(self._e.stats())
