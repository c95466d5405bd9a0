"""CPU: the launch rule of csrc/launch_rule.h - which kernel variants a batch call launches - against the launchers it replaced.
Every choice the rule makes is between kernels that return the same bytes, so no byte test sees a wrong one: here the rule's
ordered launches (kernel, grid, block) and refusals on the reduced grids of tests/launch_rule_c/grid.h are held to
tests/launch_rule_c/parent_table.txt, recorded from the former launch_decode / launch_mantx / launch_decode_wg / launch_encode
(grid.h says how).  The rule runs in tests/launch_rule_c/main.cpp, a program of its own built with the host compiler under
-fsanitize=address,undefined."""
import hashlib
import os
import re
import subprocess

import pytest

from tests import _harness as H

HERE = os.path.join(H.ROOT, "tests", "launch_rule_c")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """main.cpp built as tests/header_rule_c is -> run(mode): the lines it prints"""
    exe = str(tmp_path_factory.mktemp("launch_rule") / "launch_rule")
    H.build_sanitised([os.path.join(HERE, "main.cpp")], exe, includes=[H.CSRC])

    def run(mode):
        r = subprocess.run([exe, mode], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        return r.stdout
    return run


@pytest.fixture(scope="module")
def table():
    """parent_table.txt -> ({grid: (lines, digest)}, [spelled-out rows])"""
    sums, rows = {}, []
    for line in open(os.path.join(HERE, "parent_table.txt")).read().splitlines():
        if line.startswith("sha256 "):
            _, grid, n, digest = line.split()
            sums[grid] = (int(n), digest)
        elif not line.startswith("#"):
            rows.append(line)
    return sums, rows


def _kernels(line):
    """the launches of a canonical line -> [(kernel, 'grid x block')]"""
    return re.findall(r" ([a-z0-9_]+(?:<[^>]*>)?) (\d+x\d+);", line.split("|")[-1])


@pytest.fixture(scope="module")
def grids(program):
    return {g: program(g) for g in ("enc", "dec")}


@pytest.mark.parametrize("grid", ["enc", "dec"])
def test_rule_launches_what_the_former_launchers_did(grids, table, grid):
    """every row of the reduced grid: the same ordered (kernel, grid, block), the same refusals, and for the decoder the same
    seven front-end answers - the digest over all lines, and the table's spelled-out rows one by one (a failing digest then
    shows some of the rows that differ)"""
    sums, rows = table
    out = grids[grid]
    lines = out.splitlines()
    mine = {l.split("|")[0]: l for l in lines}
    spelled = [r for r in rows if r[0] == grid[0].upper()]
    assert len(spelled) >= 100
    differ = [(r, mine.get(r.split("|")[0])) for r in spelled if mine.get(r.split("|")[0]) != r]
    assert not differ, "recorded / rule:\n%s\n%s" % differ[0]
    assert (len(lines), hashlib.sha256(out.encode()).hexdigest()) == sums[grid]


def test_every_launch_is_listed_and_every_listed_variant_is_launched(program, grids):
    """the kernels the rule returns over both grids are exactly the variant lists' (so a launcher's table, built over its
    list, holds every word it is asked for, and the lists hold no variant that no row of the grid reaches)"""
    listed = program("lists").split("\n")[:-1]
    assert len(listed) == len(set(listed)) == 79
    seen = {k for g in grids.values() for line in g.splitlines() for k, _ in _kernels(line)}
    assert seen == set(listed), (sorted(seen - set(listed)), sorted(set(listed) - seen))


def test_thresholds(program):
    """a row on either side of each threshold differs in the expected launch and nothing else: the decoder's 512 streams and four
    frames (one workgroup per stream) and 5 120 streams (frame-parallel parse); the encoder's 1 024 frames (block packer), 2 048
    streams (tabulating search) and 5 120 streams (no launch changes: below 2 048 only does a long stream bear on the search)"""
    lines = program("pairs").splitlines()
    ks = [[k for k, _ in _kernels(l)] for l in lines]
    wg, split_fx = ["decode_wg_kernel<2, false>"], ["decode_kernel<4, true, false>", "mantx_kernel<true, true>"]
    fp = ["decode_kernel<5, false, false>", "lfsr_prefix_kernel", "mant_kernel"]
    assert ks[0:6] == [wg, split_fx, wg, fp, fp, ["decode_kernel<4, false, false>", "mant_kernel"]]
    front = ["enc_mdct_kernel<false, false, false, false, false, true>", "enc_search_kernel<1, false, false, false, true, false>"]
    assert ks[6] == front + ["enc_packb_kernel<false, false>"]
    assert ks[7] == front + ["enc_packf_kernel<true, false, false, false, false, false>"]
    plain = ["enc_mdct_kernel<false, false, false, false, false, false>", "enc_search_kernel<1, false, false, false, false, false>",
             "enc_packf_kernel<true, false, false, false, false, false>"]
    assert ks[8] == plain[:1] + ["enc_search_kernel<3, false, false, false, false, false>"] + plain[1:]
    assert ks[9] == ks[10] == ks[11] == plain
    assert all(l.endswith(" history") for l in lines[8:12]) and not any(l.endswith(" history") for l in lines[6:8])


def test_transcode_plan_takes_its_mantx_term_from_the_rule(program):
    """ac3mi_transcode_workspace_plan leaves the coefficient planes out exactly where dec_choice answers mantx for the call it
    describes (default mode, s16, no taps, a large batch): against a call of two-frame streams, which always keeps them"""
    import ctypes
    f = H.pkg().load_library().ac3mi_transcode_workspace_plan
    f.restype = ctypes.c_size_t
    f.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    answers = [tuple(int(v) for v in l.split()) for l in program("plan").splitlines()]
    assert sorted(a[:2] for a in answers) == [(1, 0), (1, 1), (2, 0), (2, 1)] and any(a[2] for a in answers)
    frames = 4096
    for fps, identity, mantx in answers:
        n_out = 6 if identity else 2
        planes = frames * 6 * 6 * 256 * 4
        assert f(frames, 3, 6, 5, n_out) - f(frames, fps, 6, 5, n_out) == (planes if mantx else 0), (fps, identity, mantx)
