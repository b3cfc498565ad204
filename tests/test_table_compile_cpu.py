"""The table compiler (csrc/table_compile.cpp) on the host: tools/table_compile_check.cpp built with
g++ (no HIP header) and run on the four fixtures, the tables at the 16-bit id boundary and their
derivations, the eager toy, and every TableOptions arm on gpt2_50k.  Per input the tool prints the
flags, masks and table sizes in clear and a 64-bit FNV-1a digest of each table's bytes, compared
with tests/golden/table_digests.json (recorded from the compiler as it stood inside load_root
before it was split into phases), and checks on the host that the tables answer for every merge
when read as csrc/pair_tables_hd.h documents them.  No GPU."""
import json
import os
import subprocess

import pytest

from tests import toys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "complexity-tokenizer_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "table_digests.json")
ARMS = ("force_wide", "no_hot_table", "no_window", "no_piece_table", "merge_slack=2", "merge16_slack=8", "piece_slack=2")


def inputs(gpt2_path, llama3_path, llama3_tt_path, multi_path, tmp_path):
    """(name, tool argument [arm:]path) of every input, each as soon as its file is written."""
    yield from {"gpt2_50k": gpt2_path, "llama3_128k": llama3_path, "llama3_tt_128k": llama3_tt_path, "multi_32k": multi_path}.items()
    for arm in ARMS:
        yield "gpt2_50k:" + arm, arm + ":" + gpt2_path

    def written(name, obj):
        path = str(tmp_path / (name + ".json"))
        with open(path, "w") as f:
            json.dump(obj, f)
        return name, path

    with open(llama3_path) as f:
        llama3 = json.load(f)
    for n in (65534, 65536, 65537):
        yield written("truncated_%d" % n, toys.truncated(llama3, n))
    base = toys.truncated(llama3, 65535)
    yield written("truncated_65535", base)
    yield written("shuffled_merges", toys.shuffled_merges(base, 1))
    yield written("invalid_merges", toys.with_invalid_merges(base, 2))
    yield written("invalid_merge_in_front", toys.with_invalid_merge_in_front(base))
    yield written("invalid_merges_tail", toys.with_invalid_merges(base, 3, tail_only=True))
    yield written("eager_cascade", toys.eager_cascade())


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    out = tmp_path_factory.mktemp("table_compile")
    exe = str(out / "table_compile_check")
    src = [os.path.join(PKG, "tools", "table_compile_check.cpp"), os.path.join(PKG, "csrc", "table_compile.cpp"),
           os.path.join(PKG, "csrc", "bpe_model.cpp")]
    objs = [str(out / (os.path.basename(c) + ".o")) for c in src]
    cc = [subprocess.Popen(["g++", "-O2", "-std=c++17", "-Wall", "-c", c, "-o", o]) for c, o in zip(src, objs)]
    assert [p.wait() for p in cc] == [0, 0, 0]
    subprocess.run(["g++", "-pthread"] + objs + ["-o", exe], check=True)
    return exe


def test_tables_match_recorded_digests_and_answer_every_merge(tool, gpt2_path, llama3_path, llama3_tt_path, multi_path, tmp_path):
    # one tool process per input, started while the later inputs are still being written
    runs = {name: subprocess.Popen([tool, arg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            for name, arg in inputs(gpt2_path, llama3_path, llama3_tt_path, multi_path, tmp_path)}
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted(runs)
    for name, p in runs.items():
        out = p.communicate()[0]
        assert p.returncode == 0, (name, out[-2000:])
        assert out.splitlines() == ["== 0"] + want[name] + ["consistent"], name


def test_inputs_reach_every_value_kind():
    """The recorded flag lines themselves: the inputs cover narrow and wide ids, compact and
    rank-valued tables, a table that is not rank-monotone (eager bits), one without window rounds,
    and one whose tier is not packed."""
    with open(GOLDEN) as f:
        want = json.load(f)

    def flags(name):
        w = want[name][0].split()
        return dict(zip(w[::2], map(int, w[1::2])))

    assert [flags("truncated_%d" % n)["narrow"] for n in (65534, 65535, 65536, 65537)] == [1, 1, 0, 0]
    assert flags("truncated_65535") == {"narrow": 1, "compact": 1, "proper": 1, "window": 1, "short_packed": 1}
    assert flags("shuffled_merges")["compact"] == 0 and flags("gpt2_50k:force_wide")["compact"] == 0
    assert flags("llama3_tt_128k")["proper"] == 0 and flags("eager_cascade")["proper"] == 0
    assert flags("invalid_merge_in_front")["window"] == 0 and flags("gpt2_50k:no_window")["window"] == 0
    assert flags("invalid_merges")["short_packed"] == 0 and flags("invalid_merges_tail")["short_packed"] == 1
