"""CPU: the native sources say only what the shipped library does.  The library reads the environment in one function
(phx_switches, phx_api.hip) and only for its two process-wide switches; every preprocessor conditional tests the device
compile or the target, or a macro the sources define unconditionally themselves -- no build-time switch of a variant."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phantom_amd", "csrc")
SWITCHES = {"PHX_AUTOTUNE", "PHX_GENERIC_SCHED"}
ALLOWED = {"__HIP_DEVICE_COMPILE__", "__gfx950__"}


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}


def _strip_comments(text):
    return re.sub(r"//[^\n]*|/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)


def _body(text, head):
    """the brace-delimited body that follows the first occurrence of `head`"""
    i = text.index("{", text.index(head))
    depth = 0
    for j in range(i, len(text)):
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i:j + 1]
    raise AssertionError(f"unbalanced braces after {head}")


def test_getenv_only_in_the_switch_reader():
    code = {f: _strip_comments(t) for f, t in _sources().items()}
    uses = {f: len(re.findall(r"\bgetenv\b", t)) for f, t in code.items()}
    reader = _body(code["phx_api.hip"], "phx_switches()")
    assert sum(uses.values()) == len(re.findall(r"\bgetenv\b", reader)) >= 1, uses
    assert set(re.findall(r'"(PHX_\w+)"', reader)) == SWITCHES


def test_conditionals_test_only_allowed_macros():
    defined, bad = set(), []
    for f, text in _sources().items():
        lines = _strip_comments(text).split("\n")
        for i, line in enumerate(lines):
            m = re.match(r"\s*#\s*define\s+(\w+)", line)
            if not m:
                continue
            prev = lines[i - 1] if i else ""
            guarded = re.match(r"\s*#\s*ifndef\s+" + m.group(1) + r"\s*$", prev)
            # a default under `#ifndef X` is a build-time switch; a bare `#define X` after it is an include guard
            if not guarded or not line[m.end():].strip():
                defined.add(m.group(1))
    for f, text in _sources().items():
        for n, line in enumerate(_strip_comments(text).split("\n"), 1):
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*)", line)
            if not m:
                continue
            names = set(re.findall(r"[A-Za-z_]\w*", m.group(2))) - {"defined"}
            for name in sorted(names - ALLOWED - defined):
                bad.append(f"{f}:{n}: {line.strip()}  ({name})")
    assert not bad, "\n".join(bad)
