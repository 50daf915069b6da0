"""The seam list of the digests of many nonces (tests/test_digests_many_host.py walks it on the host,
tests/test_gpu_digests_many.py hashes it): about 60 tasks whose seams fall after lane 0, after lane
62 and after lane 63 of a wave, on step and workgroup boundaries (entries 256 j), each of those
places also with a run of three empty tasks; the first task and the last two are empty; then 130
tasks of one entry each -- two waves of 64 different tasks and a ragged third.  Nonce lengths cycle
through NONCE_LENGTHS, so neighbouring tasks differ in p / 4, in block count and in midstate.  The
entries are test_gpu_digests.py's edge list E, in its fixed shuffled order, repeated."""
import hashlib
import random

NONCE_LENGTHS = [0, 3, 4, 7, 47, 48, 55, 56, 59, 63, 64, 119, 120, 130, 1024]

KS = [0, 1, 255, 256, 65535, 65536, 2**24 - 1, 2**24, 2**32 - 1, 2**32, 2**40 - 1, 2**40, 2**48 - 1, 2**48,
      2**55 - 2]
E = [k << 8 | tb for k in KS for tb in (0, 1, 255)]
random.Random(20240).shuffle(E)

# Where the seams of the first part fall (list positions), and whether three empty tasks sit there.
_SEAMS = [(1, True), (63, True), (64, True), (256, True), (257, False), (300, False), (319, True), (320, False),
          (321, True), (383, False), (384, False), (512, True), (517, False), (581, False), (681, False),
          (688, False), (721, False), (768, True), (769, False), (831, True), (832, False), (1000, False),
          (1024, False), (1025, False), (1087, False), (1088, True), (1150, False), (1215, False)]


def seam_lengths():
    """Segment lengths of the seam list, task by task."""
    out, at = [0], 0  # the first task is empty
    for pos, empties in _SEAMS:
        out.append(pos - at)
        at = pos
        if empties:
            out += [0, 0, 0]
    out += [0, 0]      # the last two of the first part are empty
    out += [1] * 130   # two waves of 64 different tasks, and a ragged third
    return out


def rows_of(lengths):
    rows = [0]
    for n in lengths:
        rows.append(rows[-1] + n)
    return rows


def nonce_of(nlen, salt=0):
    rnd = random.Random(7000 * nlen + salt)
    return bytes(rnd.randrange(256) for _ in range(nlen))


def seam_list():
    """(nonces, lists): task i's nonce (its length cycling through NONCE_LENGTHS, its bytes its own)
    and its entries."""
    lengths = seam_lengths()
    rows = rows_of(lengths)
    nonces = [nonce_of(NONCE_LENGTHS[i % len(NONCE_LENGTHS)], salt=i) for i in range(len(lengths))]
    lists = [[E[e % len(E)] for e in range(rows[i], rows[i + 1])] for i in range(len(lengths))]
    return nonces, lists


def secret_of(g):
    out, k = [g & 0xFF], g >> 8
    while k:
        out.append(k & 0xFF)
        k >>= 8
    return bytes(out)


def hashlib_of(nonce, indices):
    """(digests, depths) as Miner.digests returns them, from hashlib."""
    base, dig, dep = hashlib.md5(bytes(nonce)), bytearray(), bytearray()
    for g in indices:
        h = base.copy()
        h.update(secret_of(g))
        dig += h.digest()
        hx = h.hexdigest()
        dep.append(32 - len(hx.rstrip("0")))
    return bytes(dig), bytes(dep)
