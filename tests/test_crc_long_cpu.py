"""Masked CRC32C of buffers of any length, on the CPU: the model the GPU
suite's large cases rest on (tests/crc_ref.py) against the CPU codec and
outside known answers, and csrc/snapmi_crc.hpp - the cut into segments, the
search, the powers of x and the combine, compiled into a stand-alone program
(tests/crc_host.cpp, plain and with the address and undefined-behaviour
sanitizers) that computes a CRC the way the device does."""
import random
import subprocess

import pytest

import crc_ref as M
import oracle_lib as O
from conftest import ROOT

SHORT = 65536


def rand_bytes(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""


# --------------------------------------------------------------------
# 1. the model
# --------------------------------------------------------------------
def test_model_equals_the_cpu_codec():
    rng = random.Random(0xC3C)
    for n in [0, 1, 255, 256, 257, 65536, 65537, 70000]:
        d = rand_bytes(rng, n)
        c = M.crc32c(d)
        assert c == O.crc32c(d), n
        assert M.mask(c) == O.crc32c_masked(d), n


def test_model_known_answers():
    assert M.crc32c(b"123456789") == 0xE3069283
    assert M.crc32c_masked(b"123456789") == 0xC78AB0E5
    # RFC 3720 B.4
    assert M.crc32c(bytes(32)) == 0x8A9136AA
    assert M.crc32c(b"\xff" * 32) == 0x62A8AB43
    assert M.crc32c_masked(bytes(32)) == M.mask(0x8A9136AA)
    assert M.crc32c_masked(b"\xff" * 32) == M.mask(0x62A8AB43)
    assert O.crc32c_masked(bytes(32)) == M.mask(0x8A9136AA)
    assert O.crc32c_masked(b"\xff" * 32) == M.mask(0x62A8AB43)
    for c in (0, 1, 0x8A9136AA, 0xFFFFFFFF):
        assert M.unmask(M.mask(c)) == c


def test_zero_bytes_shortcut_equals_the_loop():
    # one pass of the bitwise register over 70 000 zero bytes, compared at
    # every length on the way
    c = 0xFFFFFFFF
    for n in range(70001):
        if n < 600 or n % 251 == 0 or n > 69990 or \
                n in (65535, 65536, 65537):
            assert M.crc32c_zeros(n) == c ^ 0xFFFFFFFF, n
        for _ in range(8):
            c = (c >> 1) ^ M.POLY if c & 1 else c >> 1


def test_powers_multiply():
    rng = random.Random(7)
    pairs = [(0, 0), (1, 1), (255, 1), (2**32 - 1, 1), (2**32 - 5, 70000),
             (2**32, 2**32), (2**32 + 5, 2**40 - 3), (2**40 - 1, 1),
             (2**40, 2**40 + 17), (2**63, 2**62 + 1)]
    pairs += [(rng.getrandbits(42), rng.getrandbits(34)) for _ in range(20)]
    for a, b in pairs:
        assert M.pow8(a + b) == M.gf_mul(M.pow8(a), M.pow8(b)), (a, b)
    assert M.pow8(0) == M.ONE and M.pow8(1) == M.ONE >> 8
    assert M.gf_mul(M.ONE, 0x12345678) == 0x12345678


def test_combine_equals_the_whole():
    rng = random.Random(9)
    for la, lb in [(0, 0), (0, 5), (5, 0), (1, 1), (300, 70000),
                   (65537, 255)]:
        a, b = rand_bytes(rng, la), rand_bytes(rng, lb)
        assert M.combine(M.crc32c(a), M.crc32c(b), lb) == M.crc32c(a + b)
    # ... and in whichever order the parts are joined
    x = M.crc32c(b"x" * 70000)
    assert M.combine(M.crc32c_zeros(2**32 - 69995), x, 70000) == M.combine(
        M.crc32c_zeros(2**31),
        M.combine(M.crc32c_zeros(2**31 - 69995), x, 70000),
        2**31 - 69995 + 70000)


# --------------------------------------------------------------------
# 2. the header, through a program of its own
# --------------------------------------------------------------------
DATA_BYTES = 3 * 262144 + 4096
FLAT_BYTES = 262144 + 4096


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("crc_host")
    src = str(ROOT / "tests" / "crc_host.cpp")
    plain, san = d / "crc_host", d / "crc_host_san"
    base = ["g++", "-std=c++17", "-Wall", "-Werror"]
    subprocess.check_call(base + ["-O2", src, "-o", str(plain)])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined",
                                  "-fno-sanitize-recover=all", src, "-o",
                                  str(san)])
    # random bytes, then zeros, then 0xFF: a segment of zero bytes has the
    # state 0, which the products must take like any other factor
    data = rand_bytes(random.Random(0xDA7A), DATA_BYTES) + \
        bytes(FLAT_BYTES) + b"\xff" * FLAT_BYTES
    path = d / "data.bin"
    path.write_bytes(data)

    def run(jobs):
        """The answers of both programs, which must agree, one per job."""
        text = "".join(j + "\n" for j in jobs)
        outs = []
        for exe in (plain, san):
            r = subprocess.run([str(exe), str(path)], input=text,
                               capture_output=True, text=True, timeout=60)
            assert r.returncode == 0 and not r.stderr, (exe.name, r.stderr)
            outs.append(r.stdout.splitlines())
        assert outs[0] == outs[1]
        assert len(outs[0]) == len(jobs) and "bad job" not in outs[0]
        return outs[0]
    run.data = data
    return run


def test_constants_are_the_python_side_s(host, built):
    from rust_snappy_amd import frame
    seg, short = (int(x) for x in host(["const"])[0].split())
    assert short == SHORT == frame.MAX_BLOCK_SIZE
    assert seg == frame.CRC_SEGMENT and seg % 256 == 0 and seg >= short


def test_products_with_every_kind_of_factor(host):
    rng = random.Random(0x6F)
    edge = [0, 1, M.ONE, M.ONE >> 8, 0xFFFFFFFF, M.POLY, 0x7FFFFFFF, 2]
    pairs = [(a, b) for a in edge for b in edge]
    pairs += [(rng.getrandbits(32), rng.getrandbits(32)) for _ in range(200)]
    got = host([f"mul {a} {b}" for a, b in pairs])
    for (a, b), g in zip(pairs, got):
        assert int(g, 16) == M.gf_mul(a, b) == M.gf_mul(b, a), (a, b)
    assert M.gf_mul(0, 0x12345678) == 0 == M.gf_mul(0x12345678, 0)


def test_host_program_equals_the_cpu_codec(host):
    rng = random.Random(0x5E6)
    data = host.data
    cases = []
    for seg in (256, 1024, 4096, 65536, 262144):
        # around whole numbers of segments (what is at most 64 KiB takes the
        # short route whatever the segment size)
        ks = {1, 2, 3} | ({65536 // seg, 65536 // seg + 1, 300}
                          if seg < 65536 else set())
        for k in sorted(ks):
            for n in (k * seg - 1, k * seg, k * seg + 1):
                if n <= DATA_BYTES - 3:
                    cases.append((rng.randrange(4), n, seg))
        for _ in range(30):  # and anywhere
            n = rng.choice([rng.randrange(0, 70000),
                            rng.randrange(65537, 400000),
                            rng.randrange(65537, DATA_BYTES)])
            cases.append((rng.randrange(DATA_BYTES - n + 1), n, seg))
    cases += [(0, 0, 256), (5, 0, 262144), (0, 65536, 256), (1, 65537, 256),
              (3, 65536 + 255, 256), (2, 65536 + 256, 256),
              (0, DATA_BYTES, 262144)]
    # all zeros, all 0xFF, and segments of zeros behind and in front of others
    for seg in (256, 4096, 65536, 262144):
        for base in (DATA_BYTES, DATA_BYTES + FLAT_BYTES):
            for n in (65537, 2 * seg + 65536, FLAT_BYTES - 1):
                cases.append((base + 1, min(n, FLAT_BYTES - 1), seg))
        more = min(3 * seg, FLAT_BYTES - 8)
        cases.append((DATA_BYTES - 70001, 70001 + more, seg))
        cases.append((DATA_BYTES + FLAT_BYTES - 70001, 70001 + more, seg))
    assert len(cases) >= 200
    got = host([f"crc {o} {n} {s}" for o, n, s in cases])
    for (o, n, s), g in zip(cases, got):
        assert int(g, 16) == O.crc32c_masked(data[o:o + n]), (o, n, s)


def model_plan(lens, seg):
    """first[], and every segment as (buffer, segment, off, len, tail)."""
    first, segs = [0], []
    for i, n in enumerate(lens):
        k = -(-n // seg) if n > SHORT else 0
        first.append(first[-1] + k)
        head = n - (k - 1) * seg if k else 0
        for j in range(k):
            off = 0 if j == 0 else head + (j - 1) * seg
            ln = head if j == 0 else seg
            segs.append((i, j, off, ln, n - off - ln))
    return first, segs


def test_search_with_short_and_empty_buffers_between(host):
    seg = 4096
    lists = [
        [0, 70000, 0, 0, 65536, 65537, 5, 3 * seg * 17, 0],
        [65537],
        [0, 0, 100000],
        [100000, 0, 0],
        [1, 2, 3],
        [65536 + seg, 65536 + seg + 1, 65536 + seg - 1, 0, 65536, 20 * seg],
    ]
    rng = random.Random(3)
    lists.append([rng.choice([0, 1, 65536, rng.randrange(65537, 300000)])
                  for _ in range(60)])
    for lens in lists:
        first, segs = model_plan(lens, seg)
        text = " ".join(str(n) for n in lens)
        got = host([f"first {seg} {text}"] +
                   [f"find {seg} {s} {text}" for s in range(len(segs) + 1)])
        assert [int(x) for x in got[0].split()] == first, lens
        for s, want in enumerate(segs):
            assert tuple(int(x) for x in got[1 + s].split()) == want, (lens, s)
        assert got[1 + len(segs)] == "none"
        # every byte of every long buffer is in exactly one segment
        for i, n in enumerate(lens):
            mine = [x for x in segs if x[0] == i]
            assert sum(x[3] for x in mine) == (n if n > SHORT else 0)
            assert all(0 < x[3] <= seg for x in mine)


def test_plan_arithmetic_past_32_bits(host):
    seg = 262144
    big = [2**32 - 1, 2**32, 2**32 + 5, 2**40 + 12345, 2**63 + 1, 2**64 - 1]
    got = host([f"count {seg} {n}" for n in big])
    for n, g in zip(big, got):
        k = -(-n // seg)
        assert tuple(int(x) for x in g.split()) == (k, n - (k - 1) * seg), n
    lens = [2**32 + 5, 0, 70000, 2**40 + 12345, 65536, 2**33]
    first, _ = model_plan([0], seg)
    first = [0]
    for n in lens:
        first.append(first[-1] + (-(-n // seg) if n > SHORT else 0))
    text = " ".join(str(n) for n in lens)
    assert [int(x) for x in host([f"first {seg} {text}"])[0].split()] == first
    probes = []
    for i, n in enumerate(lens):
        k = first[i + 1] - first[i]
        for j in sorted({0, 1, k // 2, k - 1} & set(range(k))):
            head = n - (k - 1) * seg
            off = 0 if j == 0 else head + (j - 1) * seg
            ln = head if j == 0 else seg
            probes.append((first[i] + j, (i, j, off, ln, n - off - ln)))
    got = host([f"find {seg} {s} {text}" for s, _ in probes])
    for (s, want), g in zip(probes, got):
        assert tuple(int(x) for x in g.split()) == want, s
    # x^(8 t) for t on both sides of 2^32 and 2^40: the model's
    ts = [0, 1, 2**32 - 1, 2**32, 2**32 + 5, 2**40 - 1, 2**40 + 7, 2**64 - 1]
    for t, g in zip(ts, host([f"pow {t}" for t in ts])):
        assert int(g, 16) == M.pow8(t), t
