"""A model of masked CRC32C in a few lines of Python - not a test.

Bitwise CRC32C (Castagnoli, reflected, polynomial 0x82F63B78), the mask of
CheckSummer::crc32c_masked, and the GF(2) arithmetic that joins the CRCs of
the parts of a message: gf_mul, x^(8 n) by squaring, the combine of two CRCs
and the CRC of n zero bytes in O(log n).  It shares nothing with the tables
of the CPU codec the suites compare with, nor with csrc/snapmi_crc.hpp.

Polynomials are in the reflected representation: bit 31 is x^0."""

POLY = 0x82F63B78
ONE = 0x80000000  # the polynomial 1
M32 = 0xFFFFFFFF


def crc32c(data, state=M32, final=M32):
    """Bit by bit: the register starts at `state`, the result is XORed with
    `final` (0xFFFFFFFF both: the CRC32C everybody means)."""
    c = state
    for b in bytes(data):
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ POLY if c & 1 else c >> 1
    return c ^ final


def mask(crc):
    """reference src/crc32.rs:35-38"""
    return (((crc >> 15) | (crc << 17)) + 0xA282EAD8) & M32


def crc32c_masked(data):
    return mask(crc32c(data))


def gf_mul(a, b):
    """a * b mod P"""
    p = 0
    for k in range(31, -1, -1):  # a's coefficients from x^0 up
        if (a >> k) & 1:
            p ^= b
        b = (b >> 1) ^ POLY if b & 1 else b >> 1  # b * x
    return p


def pow8(n):
    """x^(8 n) mod P, by squaring"""
    p, sq = ONE, ONE >> 8  # 1, x^8
    while n:
        if n & 1:
            p = gf_mul(p, sq)
        sq = gf_mul(sq, sq)
        n >>= 1
    return p


def combine(crc_a, crc_b, len_b):
    """crc32c(A + B) from crc32c(A), crc32c(B) and len(B) (what zlib calls
    crc32_combine): B's CRC carries the initial state and the final XOR of a
    message of len(B) bytes; A's, advanced past B, carries them again."""
    return gf_mul(crc_a, pow8(len_b)) ^ crc_b


def crc32c_zeros(n):
    """crc32c(bytes(n)) in O(log n): only the initial state moves."""
    return gf_mul(M32, pow8(n)) ^ M32


def unmask(m):
    c = (m - 0xA282EAD8) & M32
    return ((c >> 17) | (c << 15)) & M32
