"""Documents and the environment switch shared by tests/test_gpu_short_packed.py (pieces of
9..16 B) and tests/test_gpu_mid_packed.py (17..32 B): a few hundred short documents with pieces of
every length lo .. hi - 1 -- words over the gpt2_50k fixture's common letters (deep merges),
periodic strings (equal pairs repeated, so the leftmost rule decides), digit runs, consonant
strings (they stop merging early) -- and one document whose pieces lie across pre-tokenizer tile
ends."""
import os
import random

TILE = 3968  # bytes per pre-tokenizer tile (csrc/ctok_internal.h kTile)


def tile_end_doc(rng, lo, hi):
    """Pieces of lo .. hi - 1 B (a space and letters) starting 1, n / 2 and n - 1 bytes before a
    tile end."""
    parts, pos = [], 0
    for n in range(lo, hi):
        for delta in (1, n // 2, n - 1):
            target = (pos // TILE + 1) * TILE - delta
            if target - pos < 4:
                target += TILE
            parts.append((" ab" * (target - pos))[:target - pos])
            parts.append(" " + "".join(rng.choice("etaoinshr") for _ in range(n - 1)))
            pos = target + n
    return "".join(parts)


def docs(seed, lo, hi, reps):
    rng = random.Random(seed)
    out = [tile_end_doc(rng, lo, hi)]  # first: its offsets are the batch's
    for rep in range(reps):
        for n in range(lo, hi):  # piece length, the leading space included
            k = n - 1
            words = ["".join(rng.choice("etaoinshrdlu") for _ in range(k)) for _ in range(4)]
            words.append(("ab" * k)[:k])
            words.append(("abc" * k)[:k])
            words.append(rng.choice("aeo=-.") * k)
            words.append("".join(rng.choice("0123456789") for _ in range(k)))
            words.append("".join(rng.choice("qxzjkvwbfg") for _ in range(k)))
            words.append("".join(rng.choice("etaoinshrdlu") for _ in range(k - 1)) + rng.choice("QXZ"))
            rng.shuffle(words)
            # (the first word has no leading space: one letter more keeps it at n bytes)
            out.append(rng.choice("etaoin") + " ".join(words))
    return out


class env:
    """Sets (or with None removes) one environment variable inside a with block."""

    def __init__(self, k, v):
        self.k, self.v = k, v

    def __enter__(self):
        self.old = os.environ.get(self.k)
        if self.v is None:
            os.environ.pop(self.k, None)
        else:
            os.environ[self.k] = self.v

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop(self.k, None)
        else:
            os.environ[self.k] = self.old
