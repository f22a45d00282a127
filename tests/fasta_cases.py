"""FASTA texts for the tests of `generate --device_fasta` (test_fasta_host.py, test_gpu_fasta.py; tools/fasta_host_check.cpp holds the
same hand cases in C++): the hand cases of DESIGN.md section 31, seeded random files, and texts sized by the kernels' tile."""
import random

HAND = {
    "empty_file": b"",
    "no_header_at_all": b"ACGT\nACGT\n",
    "junk_in_front": b"junk line\nmore junk\n>a first\nACGT\nAC\n>b\nGG\n",
    "gt_inside_a_line": b">a\nAC>GT\nA>\n>b x\nTT\n",
    "header_as_last_line": b">a\nACGT\n>b no newline",
    "empty_record_between_headers": b">a\n>b\nACGT\n>c\n",
    "header_is_gt_alone": b">\nACGT\n>\n>x\nA\n",
    "crlf": b">a desc\r\nACGT\r\nAC\r\n>b\r\nGG\r\n",
    "lone_cr_inside_a_line": b">a\nAC\rGT\nA\r\n",
    "blank_lines": b"\n\n>a\n\nAC\n\n\nGT\n\n>b\n\n",
    "no_final_newline": b">a\nACGT\nACG",
    "body_with_a_space": b">a\nAC GT\n  AC\n>b\nGG\n",
    "body_with_a_tab": b">a\nAC\tGT\n>b\nGG\n",
    "body_with_a_vertical_tab": b">a\nAC\x0bGT\n>b\nGG\n",
    "body_with_a_form_feed": b">a\nAC\x0cGT\nAA\n>b\nGG\n",
    "body_with_a_high_byte": b">a\nAC\xc3\xa9GT\n>b\nGG\n",
    "body_with_a_del_byte": b">a\nAC\x7fGT\n>b\nGG\n",
    "lower_case_and_iupac": b">a\nacgtnRYKM\nswbdhvN\n>b\nNNNN\n",
    "four_tiny_records_in_16_bytes": b">\nAC\n>\nGT\n>\nTT\n>\nCA\n",
    "four_tiny_records_in_one_lane": b"thirteen junk\n>\nAC\n>\nGT\n>\nTT\n>\nCA\n",  # bytes 16 .. 31 hold letters of all four
    "header_only_file": b">only",
    "cr_before_header_is_no_line_end": b">a\nAC\r>b\nGG\n",
}


def random_file(seed, odd=None):
    """Random line widths 1 .. 200, LF and CRLF mixed, blank lines, junk in front, 1 .. 40 records of 0 .. 5 000 letters; ``odd``
    (default: every tenth seed) puts one byte outside the plain range into one body."""
    rng = random.Random(seed)
    out = bytearray()
    if rng.random() < 0.3:
        out += b"".join(rng.choice([b"junk", b" ", b"\n", b"x>y", b"\r\n"]) for _ in range(rng.randrange(1, 6)))
        if rng.random() < 0.5 and not out.endswith(b"\n"):
            out += b"\n"
    bodies = []
    for r in range(rng.randrange(1, 41)):
        eol = lambda: b"\r\n" if rng.random() < 0.3 else b"\n"  # noqa: E731
        if out and not out.endswith(b"\n"):
            out += b"\n"
        out += b">" + (b"rec%d" % r if rng.random() < 0.9 else b"") + (b" some text" if rng.random() < 0.3 else b"") + eol()
        n = rng.choice([0, 1, 2, rng.randrange(0, 200), rng.randrange(0, 5001)])
        letters = bytes(rng.choice(b"ACGTacgtNRYn") for _ in range(n))
        width, at = rng.randrange(1, 201), 0
        start = len(out)
        while at < n:
            out += letters[at:at + width] + (eol() if at + width < n or rng.random() < 0.9 else b"")
            at += width
            if rng.random() < 0.05:
                out += eol()
        bodies.append((start, len(out)))
    if odd if odd is not None else seed % 10 == 0:
        spans = [(a, b) for a, b in bodies if b > a]
        if spans:
            a, b = rng.choice(spans)
            at = rng.randrange(a, b)
            if out[at] not in b"\r\n>":
                out[at] = rng.choice(b" \t\x0b\x0c\x7f\x00\x1c")
    return bytes(out)


def letters_of(n, seed=1):
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def wrapped(letters, width, eol=b"\n"):
    return b"".join(letters[at:at + width] + eol for at in range(0, len(letters), width))


def sized(T, S):
    """Texts that put the grammar's events at the edges of a tile of T bytes and of a scan pass of S tiles: {name: bytes}."""
    out = {}
    base = b">r0\n" + wrapped(letters_of(3 * T, 2), 60)
    for n in (T - 1, T, T + 1, 2 * T + 3):
        out["length_%d" % n] = base[:n]
    for at in (T - 1, T):  # '\n' the last byte of a tile and '>' the first of the next (at = T), and one byte earlier
        head = b">a\n" + wrapped(letters_of(at, 3), 70)
        head = head[:at - 1] + b"\n"
        out["header_at_%d" % at] = head + b">b second\nACGTTGCA\nAC\n"
    out["header_line_across_an_edge"] = b">a\n" + wrapped(letters_of(T - 40, 4), 50)[:T - 23] + b"\n>" + b"h" * 40 + b" tail\nACGT\nGG\n"
    out["header_line_longer_than_a_tile"] = b">a\nAC\n>" + b"x" * (T + 100) + b"\nACGTACGT\n>c\nTT\n"
    out["body_over_three_tiles"] = b">a\nAC\n>big\n" + wrapped(letters_of(2 * T + 500, 5), 61) + b">c\nTT\n"
    for width in (1, 15, 16, 17, 60):
        out["lines_of_%d" % width] = b">w\r\n" + wrapped(letters_of(700, 6), width, b"\r\n" if width == 15 else b"\n") + b">x\nAC\n"
    for n in (S * T - 1, S * T, S * T + 1):  # the scan's second pass: a header in the last tile
        tail = b">last one\nACGTAC\nGT\n"
        body = b">first\n" + wrapped(letters_of(4000, 7), 80)
        fill = n - len(body) - len(tail)
        out["scan_span_%d" % n] = body + b">fill\n" + (b"ACGTTGCA" * (fill // 8 + 1))[:fill - 7] + b"\n" + tail
        assert len(out["scan_span_%d" % n]) == n
    return out


def bgzf(data, block=700):
    """BGZF members of ``block`` bytes each and the EOF block, made with zlib."""
    import struct
    import zlib

    out = bytearray()
    for at in list(range(0, len(data), block)) + [None]:
        piece = data[at:at + block] if at is not None else b""
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        pay = z.compress(piece) + z.flush()
        out += b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(pay) + 25)
        out += pay + struct.pack("<II", zlib.crc32(piece), len(piece))
    return bytes(out)
