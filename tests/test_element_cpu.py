"""The reference's element loop on the CPU: csrc/snapmi_element.hpp compiled
into a stand-alone program (tests/element_host.cpp) that runs lane_decode -
the prologue and the element loop that the lane kernels run on global memory
- over plain host memory, on whole streams and on their elements as a
headerless piece, and the walker.  Output length, output bytes, error kind
and the three fields are compared with snapo_decompress of the oracle, the
walker with tests/indexbuild_ref.py's elem_step, stream by stream: the
reference's KATs, the golden raw vector, the corpus, the blocks of
token_shapes.py, every truncation of three short streams and a few thousand
single-byte corruptions.  The same program runs once more with
-fsanitize=address,undefined.  The error variants that the GPU suite sends to
every decoder (tests/error_variants.py) are held to their conditions here.

What this does NOT run: the staged loop of k_decompress_tiny / _small and
decode_sequential keep lane_decode's checks written out (registers:
profiles/decoder_split_resources.md); an edit to those copies fails the GPU
suite (test_error_kats_on_every_decoder and the parity tests), not this
file."""
import random
import struct
import subprocess
import zlib

import pytest

import error_variants as V
import indexbuild_ref as IB
import kats
import oracle_lib as O
import token_shapes as T
from conftest import ROOT


def cap_of(data):
    try:
        return O.decompress_len(data)
    except O.SnapError:
        return 1024


def streams():
    out = [(name, data) for name, data, _ in kats.DECODE_KATS]
    out += [(name, data) for name, data, _, _ in kats.ERROR_KATS]
    out.append(("golden", (O.CORPUS / "Mark.Twain-Tom.Sawyer.txt.rawsnappy")
                .read_bytes()))
    for bench_id, data in O.corpus_round():
        out.append((bench_id, O.compress(data[:65536])))
    out += [(c.name, c.comp) for c in T.the_set().single_blocks()]
    short = [O.compress(b"aaaa" + b"b" * 9 + b"aaaabbbb"),
             O.compress(bytes(range(70)) + bytes(range(70))),
             kats.DECODE_KATS[0][1]]
    for i, s in enumerate(short):
        out += [("trunc-%d-%d" % (i, n), s[:n]) for n in range(len(s))]
    rng = random.Random(20)
    base = short + [O.compress(d[:300]) for _, d in O.corpus_round()[:6]] + [
        O.compress(d[2000:6000]) for _, d in O.corpus_round()[:4]]
    for k in range(3000):
        b = bytearray(rng.choice(base))
        b[rng.randrange(len(b))] = rng.randrange(256)
        out.append(("corrupt-%d" % k, bytes(b)))
    for cls in V.CLASSES[:4]:
        out += [("%s-%s" % (cls, name), comp)
                for name, _, comp in V.variants(cls)]
    return out


STREAMS = streams()


def build(tmp, name, extra):
    exe = tmp / name
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror"]
                          + extra
                          + [str(ROOT / "tests" / "element_host.cpp"),
                             "-o", str(exe)])
    return exe


def run(exe, tmp, cases):
    path = tmp / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for _, data in cases:
            f.write(struct.pack("<QI", cap_of(data), len(data)) + data)
    out = subprocess.run([str(exe), str(path)], capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 3 * len(cases)
    return [lines[3 * i:3 * i + 3] for i in range(len(cases))]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("element"), "element_host", [])


@pytest.fixture(scope="module")
def answers(exe, tmp_path_factory):
    return run(exe, tmp_path_factory.mktemp("element_cases"), STREAMS)


def oracle_line(data):
    """kind a b c out_len crc, as the host program prints a decode."""
    try:
        out = O.decompress(data, cap_of(data))
        return "0 0 0 0 %d %d" % (len(out), zlib.crc32(out))
    except O.SnapError as e:
        return "%d %d %d %d 0 %d" % (e.kind, e.a, e.b, e.c, zlib.crc32(b""))


def test_lane_decode_is_the_oracle(answers):
    kinds = set()
    pieces = 0
    for (name, data), lines in zip(STREAMS, answers):
        want = oracle_line(data)
        kinds.add(want.split()[0])
        assert lines[0] == "flat " + want, name
        # header and capacity passed: the piece is the same decode
        if lines[1] != "piece -":
            assert lines[1] == "piece " + want, name
            pieces += 1
        else:
            assert want.split()[0] in ("1", "2", "3", "4"), name
    # every kind the element loop and the prologue can report was met
    assert kinds >= {str(k) for k in (0, 1, 3, 4, 5, 6, 7, 8, 9)}
    assert pieces > len(STREAMS) // 2


def test_walker_is_indexbuild_refs(answers):
    for (name, data), lines in zip(STREAMS, answers):
        try:
            hdr, _ = V.header(data)
        except ValueError:
            assert lines[2] == "walk -", name
            continue
        if hdr > 10:       # more than 64 bits: no header either
            assert lines[2] == "walk -", name
            continue
        p, out, n, ok = hdr, 0, 0, True
        while ok and p < len(data):
            step = IB.elem_step(data, p, out)
            if step is None:
                ok = False
            else:
                (p, out), n = step, n + 1
        assert lines[2] == "walk %d %d %d %d" % (ok, p, out, n), name


def test_tag_table_is_the_walkers(exe):
    """tag_encoded / tag_produced (what hop_lut tabulates) against one hop
    of the reference walker over the tag and enough bytes behind it."""
    out = subprocess.run([str(exe), "tags"], capture_output=True, text=True)
    assert out.returncode == 0
    lines = out.stdout.splitlines()
    assert len(lines) == 256
    for t, ln in enumerate(lines):
        if t & 3 == 0 and (t >> 2) >= 60:
            assert ln == "%d 0 0" % t          # length bytes follow
        else:
            p, produced = IB.elem_step(bytes([t]) + bytes(80), 0, 0)
            assert ln == "%d %d %d" % (t, p, produced)


def test_sanitizers_clean(tmp_path, answers):
    """The same program with -fsanitize=address,undefined gives the same
    answer and exits clean: every buffer is an allocation of its exact size."""
    exe = build(tmp_path, "element_host_san",
                ["-g", "-fsanitize=address,undefined",
                 "-fno-sanitize-recover=all"])
    assert run(exe, tmp_path, STREAMS) == answers


# ---- the error variants of tests/test_gpu_parity.py ------------------------
@pytest.mark.parametrize("cls", V.CLASSES)
def test_error_variants_keep_their_kind_and_their_class(cls):
    names = [name for name, _, _ in V.variants(cls)]
    left = V.LEFT_OUT.get(cls, {})
    assert len(left) <= 2
    want_names = [k[0] for k in V.parsing_kats() if k[0] not in left]
    if cls == "seq":
        left = V.LEFT_OUT.get("wide", {})
        want_names = [k[0] for k in V.parsing_kats()] + [
            k[0] for k in V.parsing_kats() if k[0] not in left]
    assert names == want_names             # no other KAT is left out
    for name, kind, comp in V.variants(cls):
        with pytest.raises(O.SnapError) as e:
            O.decompress(comp, O.decompress_len(comp))
        assert e.value.name == kind, (cls, name)
        if cls != "seq":
            assert V.in_class(cls, comp), (cls, name, len(comp))


def test_left_out_kats_do_change_their_kind():
    """The reason a KAT is left out of a class is real: with that class's
    prefix its copy is valid and another check fails."""
    for cls, left in V.LEFT_OUT.items():
        for name in left:
            data = next(k[1] for k in V.parsing_kats() if k[0] == name)
            comp = V.variant(cls, data)
            with pytest.raises(O.SnapError) as e:
                O.decompress(comp, O.decompress_len(comp))
            assert e.value.name != "Offset"
