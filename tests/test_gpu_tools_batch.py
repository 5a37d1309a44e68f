"""tools/szip given several files: runs of small files go through one
snapmi_frame_compress_batch_host / snapmi_frame_decompress_batch_host call on
one context, larger files through the pipeline - and nothing a user can
observe differs from one invocation per file: output names and bytes, -k / -f
/ -v, one message per failing file in argument order, the exit status."""
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SZIP = ROOT / "tools" / "szip"
THRESHOLD = 1 << 20        # kBatchBelow of tools/szip.cpp


def run(args, **kw):
    return subprocess.run([str(SZIP)] + [str(a) for a in args],
                          capture_output=True, timeout=300, **kw)


def make_files(d):
    """40 small files (0 bytes .. 300 KB: one and several chunks) and one
    above the threshold, which sits in the middle of the arguments."""
    t = b"".join((O.CORPUS / n).read_bytes()
                 for n in ("alice29.txt", "lcet10.txt", "plrabn12.txt"))
    sizes = [0, 1, 100, 4096, 65535, 65536, 65537, 300_000] + \
        [1000 + 2777 * k for k in range(32)]
    files = []
    for k, n in enumerate(sizes):
        f = d / f"f{k:02d}.txt"
        f.write_bytes(t[31 * k:31 * k + n])
        files.append(f)
    big = d / "big.bin"
    big.write_bytes(t[:THRESHOLD + 12345])
    files.insert(20, big)
    assert len(files) == 41 and big.stat().st_size >= THRESHOLD
    return files


def test_many_files_equal_one_invocation_each(built, tmp_path):
    files = make_files(tmp_path)
    datas = [f.read_bytes() for f in files]
    p = run(["-k"] + files)
    assert p.returncode == 0 and p.stderr == b"", p.stderr
    got = [Path(str(f) + ".sz").read_bytes() for f in files]
    # each file in its own invocation (a few at a time)
    alone = tmp_path / "alone"
    alone.mkdir()
    for f, d in zip(files, datas):
        (alone / f.name).write_bytes(d)
    with ThreadPoolExecutor(max_workers=8) as ex:
        res = list(ex.map(lambda f: run(["-k", alone / f.name]), files))
    assert all(r.returncode == 0 for r in res)
    for f, g, d in zip(files, got, datas):
        assert g == (alone / (f.name + ".sz")).read_bytes(), f.name
        assert g == O.frame_compress(d), f.name
        assert f.exists()                                  # -k
        assert abs(Path(str(f) + ".sz").stat().st_mtime
                   - f.stat().st_mtime) < 2                # times preserved
    # -d restores them and removes the .sz files (no -k)
    for f in files:
        f.unlink()
    q = run(["-d"] + [str(f) + ".sz" for f in files])
    assert q.returncode == 0 and q.stderr == b"", q.stderr
    for f, d in zip(files, datas):
        assert f.read_bytes() == d, f.name
        assert not Path(str(f) + ".sz").exists()


def test_one_corrupt_file_among_many(built, tmp_path):
    import rust_snappy_amd as R
    files = make_files(tmp_path)
    datas = [f.read_bytes() for f in files]
    assert run(files).returncode == 0
    assert not any(f.exists() for f in files)              # removed like gzip
    szs = [Path(str(f) + ".sz") for f in files]
    bad = szs[7]                                           # 300 000 bytes
    framed = bytearray(bad.read_bytes())
    framed[len(framed) - 200] ^= 0xFF                      # in the last chunk
    bad.write_bytes(bytes(framed))
    with pytest.raises(O.SnapError) as oe:
        O.frame_decompress(bytes(framed))
    e = oe.value
    text = R.error.Error(e.kind, e.a, e.b, e.c).display()
    # and a file that is not there, and one that is not .sz: messages in
    # argument order, one each
    stray = tmp_path / "stray.txt"
    stray.write_bytes(b"x")
    args = szs[:3] + [tmp_path / "missing.sz"] + szs[3:30] + [stray] + szs[30:]
    p = run(["-d", "-k"] + args)
    assert p.returncode == 1
    lines = p.stderr.decode().splitlines()
    assert len(lines) == 3, lines
    assert "missing.sz" in lines[0]
    assert lines[1] == f"szip: {bad}: {text}"
    assert lines[2] == f"szip: {stray}: skipping uncompressed file"
    for f, sz, d in zip(files, szs, datas):
        assert sz.exists()                                 # -k
        if sz == bad:
            assert not f.exists()
        else:
            assert f.read_bytes() == d, f.name
    # the same through the pipeline, one file: the same message
    q = run(["-d", "-k", bad])
    assert q.returncode == 1
    assert q.stderr.decode().splitlines() == [lines[1]]
    # without -f nothing is overwritten: one message per file
    r = run(["-d", "-k"] + szs[:5])
    assert r.returncode == 1
    assert r.stderr.decode().splitlines() == [
        f"szip: skipping, file already exists: {f}" for f in files[:5]]
    assert run(["-d", "-k", "-f"] + szs[:5]).returncode == 0
    # -v: one line per file
    v = run(["-d", "-k", "-f", "-v"] + szs[:5])
    assert v.returncode == 0
    vl = v.stderr.decode().splitlines()
    assert len(vl) == 5
    for f, sz, line in zip(files, szs, vl):
        assert line.startswith(f"szip: {sz}: ") and "GiB/s" in line
