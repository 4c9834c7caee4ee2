"""bzip2 inputs for the block-parallel decode tests, made with Python's bz2 (libbz2) at level 1, where a block holds 100 000
bytes, so that the shapes stay small: empty, one byte, one block, three blocks with starts at unaligned bit offsets, the
run-length layer in front of the BWT at its edges, every byte value, a one-symbol alphabet."""
import bz2
import random


def fastq(n_bytes=250_000, seed=11):
    """seeded FASTQ with ACGT bases and random qualities (no runs to speak of: the blocks hold what they say)"""
    rng = random.Random(seed)
    out, size, i = [], 0, 0

    def rec(name, k):
        return b"@%s\n%s\n+\n%s\n" % (name, bytes(rng.choice(b"ACGT") for _ in range(k)), bytes(rng.randint(33, 73) for _ in range(k)))
    while size + 1000 < n_bytes:
        out.append(rec(b"read%05d" % i, rng.randint(100, 400)))
        size += len(out[-1])
        i += 1
    # the last record fills the text to n_bytes exactly: 2 k + 6 + the name's length
    rest = n_bytes - size
    name = b"read%05d" % i + (b"" if (rest - 6 - 9) % 2 == 0 else b"x")
    out.append(rec(name, (rest - 6 - len(name)) // 2))
    text = b"".join(out)
    assert len(text) == n_bytes
    return text


def noise(n, seed):
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGTNacgtn0123456789") for _ in range(n))


def plains():
    fq = fastq()
    runs = b"".join(bytes([65 + i]) * k + b"." for i, k in enumerate((4, 5, 255, 259, 260, 3, 8, 1000, 256)))
    return [
        ("empty", b""),
        ("one_byte", b"x"),
        ("one_block", fastq(60_000, 12)),
        ("three_blocks", fq),
        ("runs", runs),
        ("run_over_block_boundary", noise(99_900, 1) + b"G" * 300 + noise(1000, 2)),
        ("block_ends_inside_run", noise(99_970, 3) + b"C" * 40 + noise(500, 4)),
        ("ends_with_run_of_4", noise(500, 5) + b"T" * 4),
        ("ends_inside_long_run", noise(500, 6) + b"T" * 700),
        ("all_bytes", bytes(range(256)) * 8 + bytes(reversed(range(256)))),
        ("one_symbol", b"A" * 5000),
        ("zeros", bytes(100_000)),
    ]


_CASES = None


def cases():
    """(name, bzip2 bytes, plain bytes); computed once"""
    global _CASES
    if _CASES is None:
        out = [(name, bz2.compress(p, 1), p) for name, p in plains()]
        fq = fastq()
        out.append(("three_blocks_as_one_l9", bz2.compress(fq, 9), fq))
        _CASES = out
    return _CASES


def three_blocks():
    return next(c for c in cases() if c[0] == "three_blocks")
