"""Every error KAT (tests/kats.py) restated so that it lands on each of the
decoder's restatements of the reference's loop: a prefix of valid elements is
put in front of the KAT's elements and the varint rewritten to dlen + what
the prefix produces.  The prefix moves the KAT's failing element to another
place of the stream - and the stream to another kernel - without changing
which check fails; tests/test_element_cpu.py holds every variant against the
oracle (its error has the KAT's kind), tests/test_gpu_parity.py sends them to
the GPU.

The classes (csrc/snapmi_decompress.hip, plan_class):
  lds     under 256 compressed bytes, output of at most 256: k_decompress_tiny
          on its staged loop
  short_wide  under 256 compressed bytes announcing more than 256 bytes of
          output: not the staged loop's - plan_class gives it to the wavefront
          decoder, like `wide`, with almost no input in front of the failing
          element.  (lane_decode on global memory runs for headerless pieces
          and stored chunks only; no raw stream reaches it with an element
          error.  The CPU suite runs it on all of these bytes.)
  small   256 .. 511 compressed bytes, output of at most 512:
          k_decompress_small
  wide    512 compressed bytes and more: the wavefront decoder, whose window
          loops hand over to decode_sequential
  seq     decode_kernel 0: k_decompress_sequential (the streams of `lds` and
          of `wide`)

The prefix is ONE literal of N bytes wherever that can do it.  For `short_wide`
it cannot for the KATs that announce 2 or 5 bytes: a literal of N bytes
occupies more than N, so compressed < 256 and dlen + N > 256 need dlen > 6;
those get a literal of 8 bytes and four copies of 64 from it (264 bytes of
output in 21), still nothing but valid elements in front.
"""
import kats


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def header(data):
    """(header bytes, dlen) of a KAT whose header parses."""
    v = shift = 0
    for i, b in enumerate(data):
        v |= (b & 0x7F) << shift
        shift += 7
        if b < 0x80:
            return i + 1, v
    raise ValueError("no header")


def literal(n, fill=0x41):
    body = bytes((fill + k) & 0xFF for k in range(n))
    if n <= 60:
        return bytes([(n - 1) << 2]) + body
    if n <= 256:
        return bytes([60 << 2, n - 1]) + body
    assert n <= 65536
    return bytes([61 << 2]) + (n - 1).to_bytes(2, "little") + body


def literal_and_copies():
    """8 literal bytes, then four copy-2 elements of 64 bytes at offset 8:
    (elements, bytes produced)."""
    copy = bytes([((64 - 1) << 2) | 2, 8, 0])
    return literal(8) + copy * 4, 8 + 4 * 64


def with_prefix(data, elements, produced):
    hdr, dlen = header(data)
    return varint(dlen + produced) + elements + data[hdr:]


LITERAL_N = {"lds": 20, "small": 300, "wide": 600}

# KATs a class cannot hold, with the reason (at most two per class)
LEFT_OUT = {
    # the copy's offset of 255 must reach in front of the output's start: the
    # KAT's element has to stand within 254 bytes of it, and 256 compressed
    # bytes of literal in front of it produce more
    "small": {"err_copy_offset_big":
              "offset 255 is valid behind 256 bytes of output"},
    "wide": {"err_copy_offset_big":
             "offset 255 is valid behind 512 bytes of output"},
}


def parsing_kats():
    return [k for k in kats.ERROR_KATS if not k[3] and k[1]]


def unchanged_kats():
    """Bad headers and the empty stream: no header to rewrite."""
    return [k for k in kats.ERROR_KATS if k[3] or not k[1]]


def variant(cls, data):
    if cls == "short_wide":
        hdr, dlen = header(data)
        body = len(data) - hdr
        # the longest literal that keeps the stream under 256 bytes
        n = 255 - body - 2 - len(varint(dlen + 250))
        n = min(n, 253)    # (a copy of offset 255 must still reach too far)
        if dlen + n > 256:
            return with_prefix(data, literal(n), n)
        return with_prefix(data, *literal_and_copies())
    n = LITERAL_N[cls]
    return with_prefix(data, literal(n), n)


def in_class(cls, comp):
    """Does `comp` (a variant) land where the class says?  By plan_class's
    rules on the stream's lengths."""
    hdr, dlen = header(comp)
    n = len(comp)
    if cls == "lds":
        return n < 256 and dlen <= 256
    if cls == "short_wide":
        return n < 256 and dlen > 256
    if cls == "small":
        return 256 <= n < 512 and dlen <= 512
    return n >= 512


def variants(cls):
    """[(KAT name, KAT kind, stream)] of a class; `seq` is lds + wide."""
    if cls == "seq":
        return variants("lds") + variants("wide")
    out = []
    for name, data, want, _ in parsing_kats():
        if name in LEFT_OUT.get(cls, {}):
            continue
        out.append((name, want[0], variant(cls, data)))
    return out


CLASSES = ("lds", "short_wide", "small", "wide", "seq")
