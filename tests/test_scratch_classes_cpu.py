"""Every DevBuf / PinBuf a context owns says at its declaration whether it is
scratch (every word a call reads was written earlier in the same call) or
kept (meaning survives a call), and DESIGN.md 4.2b lists each with that class
and, for a kept one, the site that initialises it.  This test parses the
declarations of snapmi_ctx.hpp and snapmi_hostpipe.hpp and holds the table to
them: a buffer added without a class, or without a row, fails here, before
tests/test_gpu_scratch.py has to find out on a GPU what it reads."""
import re

from conftest import ROOT

CSRC = ROOT / "rust-snappy_amd" / "csrc"
CLASSES = {"ScratchDev": "scratch", "ScratchPin": "scratch",
           "KeptDev": "kept", "KeptPin": "kept"}
# the pinned words that are no PinBuf: kept by definition, listed too
PINNED_WORDS = {"h_mail", "h_ratio", "h_tokstat", "PipeSlot::h_res",
                "PipeSlot::h_off"}
# a struct's members are named with the struct, the context's plainly
PREFIX = {"snapmi_ctx": "", "UpdateScratch": "UpdateScratch::",
          "PipeSlot": "PipeSlot::"}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _struct_body(text, name):
    # (the definition: a base list may stand before the brace)
    m = re.search(r"\bstruct\s+%s\s*(?::[^;{]*)?\{" % re.escape(name), text)
    assert m, f"struct {name} not found"
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[m.end():i - 1]


def declared():
    """{name: class} of every buffer member, and the list of members declared
    with a bare DevBuf / PinBuf (no class)."""
    found, bare = {}, []
    for path, structs in ((CSRC / "snapmi_ctx.hpp",
                           ("UpdateScratch", "snapmi_ctx")),
                          (CSRC / "snapmi_hostpipe.hpp", ("PipeSlot",))):
        text = _strip_comments(path.read_text())
        for st in structs:
            body = _struct_body(text, st)
            for m in re.finditer(
                    r"(?<![\w:<*])(?:snapmi::)?"
                    r"(DevBuf|PinBuf|ScratchDev|ScratchPin|KeptDev|KeptPin)"
                    r"\s+([^;()<>*&]+);", body):
                kind, names = m.group(1), m.group(2)
                for n in names.split(","):
                    n = re.sub(r"\[[^\]]*\]", "", n).strip()
                    assert re.fullmatch(r"\w+", n), (st, m.group(0))
                    full = PREFIX[st] + n
                    if kind in CLASSES:
                        assert full not in found, f"{full} declared twice"
                        found[full] = CLASSES[kind]
                    else:
                        bare.append(full)
    return found, bare


def table():
    """[(name, class, site)] of the rows of DESIGN.md 4.2b."""
    text = (ROOT / "DESIGN.md").read_text()
    m = re.search(r"^### 4\.2b [^\n]*\n(.*?)^### ", text, flags=re.S | re.M)
    assert m, "DESIGN.md has no section 4.2b"
    rows = []
    for line in m.group(1).splitlines():
        r = re.match(r"\|\s*`([^`]+)`\s*\|\s*(\w+)\s*\|\s*(.*?)\s*\|\s*$", line)
        if r:
            rows.append(r.groups())
    return rows


def test_every_buffer_is_declared_with_a_class():
    found, bare = declared()
    assert not bare, f"declared without a class: {bare}"
    # the parser sees what the headers hold: the known corners of each struct
    for name in ("blk_first", "order", "pin_desc", "pin_ibg", "fr_nowait",
                 "UpdateScratch::stat", "UpdateScratch::pin", "PipeSlot::in",
                 "PipeSlot::hb_home"):
        assert found.get(name) == "scratch", name
    for name in ("lane_tables", "lane_epochs", "ix_gate", "fr_tables"):
        assert found.get(name) == "kept", name
    assert len(found) >= 55


def test_nothing_else_holds_a_bare_buffer():
    """The classes are the only way to own a buffer: outside the two base
    types' own definitions no file of the library declares a DevBuf or a
    PinBuf by value (references, pointers and parameters aside)."""
    for path in sorted(CSRC.glob("*.h*")):
        text = _strip_comments(path.read_text())
        for m in re.finditer(r"(?<![\w:<*])(?:snapmi::)?(DevBuf|PinBuf)\s+"
                             r"(\w+)\s*(?:,\s*\w+\s*)*;", text):
            raise AssertionError(f"{path.name}: {m.group(0)!r} has no class")


def test_design_table_matches_the_declarations():
    found, _ = declared()
    rows = table()
    names = [r[0] for r in rows]
    twice = {n for n in names if names.count(n) > 1}
    assert not twice, f"listed twice: {sorted(twice)}"
    by_name = {n: (c, site) for n, c, site in rows}
    missing = sorted(set(found) - set(by_name))
    assert not missing, f"declared but not in DESIGN.md 4.2b: {missing}"
    unknown = sorted(set(by_name) - set(found) - PINNED_WORDS)
    assert not unknown, f"in DESIGN.md 4.2b but not declared: {unknown}"
    for n, cls in found.items():
        assert by_name[n][0] == cls, (n, cls, by_name[n][0])
        assert len(by_name[n][1]) > 10, f"{n}: no writing / initialising site"
    for n in PINNED_WORDS:
        assert n in by_name and by_name[n][0] == "kept", n
        assert len(by_name[n][1]) > 10, n


def test_the_pinned_words_exist():
    """... under the names the table gives them."""
    ctx = _strip_comments((CSRC / "snapmi_ctx.hpp").read_text())
    pipe = _strip_comments((CSRC / "snapmi_hostpipe.hpp").read_text())
    for n in ("h_mail", "h_ratio", "h_tokstat"):
        assert re.search(r"\*\s*%s\b" % n, _struct_body(ctx, "snapmi_ctx")), n
    for n in ("h_res", "h_off"):
        assert re.search(r"\*\s*%s\b" % n, _struct_body(pipe, "PipeSlot")), n


def test_reserves_see_the_class():
    """reserve, pin_reserve and slot_reserve take the base types, which carry
    the class in `kept`, and hand every new allocation to the test build's
    fill."""
    ctx = (CSRC / "snapmi_ctx.hpp").read_text()
    assert re.search(r"struct KeptDev : DevBuf \{\s*KeptDev\(\) \{ kept = true; \}",
                     ctx)
    assert re.search(r"struct KeptPin : PinBuf \{\s*KeptPin\(\) \{ kept = true; \}",
                     ctx)
    for path, func, fill in (("snapmi_ctx.hpp", "inline int reserve(",
                              "fill_new_dev(ctx, b)"),
                             ("snapmi_launch.hpp", "inline int pin_reserve(",
                              "fill_new_pin(ctx, b)"),
                             ("snapmi_hostpipe.hip", "int snapmi::slot_reserve(",
                              "fill_new_dev(ctx, b)"),
                             ("snapmi_hostbatch.hip", "int pin_buf(",
                              "fill_new_pin(ctx, b)")):
        text = (CSRC / path).read_text()
        at = text.index(func)
        body = text[at:text.index("\n}\n", at)]
        assert fill in body, (path, func)
        assert "#ifdef SNAPMI_TESTING" in body, (path, func)
