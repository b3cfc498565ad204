"""Tables and texts at the 16-bit id boundary (shared by tests/test_native_cpu.py and
tests/test_gpu_id16_boundary.py).

The host narrows ids to 16 bits when the largest model-vocab id is below 0xFFFF (0xFFFF is the
sentinel of the u16 token slots, merge values and piece records): tables of 65,534 and 65,535 ids
are narrow, 65,536 and 65,537 are not.  They are prefixes of the llama3_128k fixture
(toys.truncated).  The corpus puts the highest ids of such a table into pieces of every length
class, so that id 0xFFFE (and merge value 0xFFFE: the tables are compact) goes through every
merge tier, the piece records and the u16 wire.
"""
import copy
import random

from oracle import ref_c
from tests import toys

N_IDS = (65534, 65535, 65536, 65537)
TOP_K = 64
SUFFIX_LENS = (1, 2, 3, 5, 8, 12, 20, 30, 50, 90, 300)
TILE = 3968  # bytes per pre-tokenizer tile (csrc/ctok_internal.h kTile)
CLASSES = ("<= 8 B", "9..16 B", "17..32 B", "33..64 B", "> 64 B")
# added tokens that can match inside a piece, with ids at and past the 16-bit range
ADDED_IDS = {"ing": 65535, "ll": 65536, "zz": 70000}


def length_class(n):
    return 0 if n <= 8 else 1 if n <= 16 else 2 if n <= 32 else 3 if n <= 64 else 4


def token_bytes(tok):
    """The raw bytes of a byte-level token string."""
    inv = {c: b for b, c in enumerate(toys.byte_map())}
    return bytes(inv[c] for c in tok)


def top_texts(obj, k=TOP_K):
    """The texts of the table's k highest ids (those that are valid UTF-8: all of them in the
    llama3 fixture's range used here), highest first."""
    inv = {i: t for t, i in obj["model"]["vocab"].items()}
    n = max(inv) + 1
    return [token_bytes(inv[i]).decode("utf-8") for i in range(n - 1, n - 1 - k, -1)]


def boundary_docs(obj, reps=6, seed=3):
    """One word per document: the text of one of the top ids and a random letter suffix, so the
    word's merges start from a top id's own merges and go on through the tier of its length."""
    rng = random.Random(seed)
    docs = []
    for _ in range(reps):
        for t in top_texts(obj):
            for n in SUFFIX_LENS:
                docs.append(t + "".join(rng.choice("etaoinshrdlu") for _ in range(n)))
    return docs


def tile_end_doc(obj, seed=5):
    """The same kind of words in one document, each placed so that it starts 1, n / 2 or n - 1
    bytes before a pre-tokenizer tile end (filler in between)."""
    rng = random.Random(seed)
    tops = top_texts(obj)
    parts, pos = [], 0
    for k, n_suffix in enumerate((1, 3, 5, 8, 12, 20, 30, 50)):
        for which in range(3):
            word = tops[(3 * k + which) % len(tops)] + "".join(rng.choice("etaoinshrdlu") for _ in range(n_suffix))
            word = word if word.startswith(" ") else " " + word
            n = len(word.encode())
            delta = (1, n // 2, n - 1)[which]
            target = (pos // TILE + 1) * TILE - delta
            if target - pos < 4:
                target += TILE
            parts.append((" ab" * (target - pos))[:target - pos])
            parts.append(word)
            pos = target + n
    return "".join(parts)


def with_added_ids(obj, ids=None, single_word=False):
    """obj + added tokens that can match inside a piece, with the given ids."""
    out = copy.deepcopy(obj)
    out["added_tokens"] = list(out.get("added_tokens", [])) + [
        {"id": i, "content": c, "single_word": single_word, "lstrip": False, "rstrip": False, "normalized": False,
         "special": False} for c, i in (ADDED_IDS if ids is None else ids).items()]
    return out


def spliced_docs(docs, seed=7):
    """Every third document gets one of the added contents put inside its word ("ll" also occurs
    in the random suffixes by itself)."""
    rng = random.Random(seed)
    out = []
    for k, d in enumerate(docs):
        if k % 3 == 0:
            c = rng.choice(sorted(ADDED_IDS))
            p = rng.randrange(1, len(d) + 1)
            d = d[:p] + c + d[p:]
        out.append(d)
    return out


def class_counts(docs, ids, off, n_ids):
    """Per length class, among the documents that are a single multi-token piece: how many hold
    the top id n_ids - 1, and how many hold an id >= n_ids - 64 (ids, off: an encoder's output for
    docs)."""
    top = [0] * 5
    near = [0] * 5
    o = [int(x) for x in off]
    for k, d in enumerate(docs):
        b = d.encode()
        got = ids[o[k]:o[k + 1]]
        if len(got) < 2 or len(ref_c.pieces(b)) != 1:
            continue
        c = length_class(len(b))
        mx = int(got.max())
        top[c] += mx == n_ids - 1
        near[c] += mx >= n_ids - 64
    return top, near


def assert_reaches_every_class(docs, ids, off, n_ids):
    """The precondition of the boundary tests, on the oracle's output: in every length class some
    multi-token piece contains the top id, and at least 100 contain one of the top 64."""
    top, near = class_counts(docs, ids, off, n_ids)
    for c, name in enumerate(CLASSES):
        assert top[c] >= 1 and near[c] >= 100, "%s: %d pieces with id %d, %d with an id >= %d" % (
            name, top[c], n_ids - 1, near[c], n_ids - 64)
    return top, near


def expected_props(obj, added_in_piece_ids=()):
    """The load-time properties by the rules the loader states (csrc/ctok_host.cpp: `narrow`: every
    vocab id below 0xFFFF; `compact`: new id strictly increasing in rank over the merges that can
    merge; `short_packed`: narrow, compact, no entry whose lookup panics and every table value
    below 0xFFFF; `ids16`: narrow and every added token that can match inside a piece below
    0xFFFF), restated on the tokenizer.json object: merges whose parts or result are missing from
    the vocab are skipped but keep their rank (src/bpe.rs:60-69), a rank past the number of valid
    merges panics when looked up, and a table value is the new id of the valid merge at index
    rank."""
    vocab = obj["model"]["vocab"]
    ranks, valid_new = {}, []
    for r, m in enumerate(obj["model"]["merges"]):
        a, b = m.split(" ") if isinstance(m, str) else m
        if a in vocab and b in vocab and a + b in vocab:
            ranks[(vocab[a], vocab[b])] = r
            valid_new.append(vocab[a + b])
    narrow = max(vocab.values()) < 0xFFFF
    live = sorted(r for r in ranks.values() if r < len(valid_new))
    compact = all(valid_new[x] < valid_new[y] for x, y in zip(live, live[1:]))
    panics = any(r >= len(valid_new) for r in ranks.values())
    values = [valid_new[r] for r in live]
    short_packed = narrow and compact and not panics and all(v < 0xFFFF for v in values)
    ids16 = narrow and all(i < 0xFFFF for i in added_in_piece_ids)
    return {"narrow": narrow, "compact": compact, "short_packed": short_packed, "ids16": ids16}
