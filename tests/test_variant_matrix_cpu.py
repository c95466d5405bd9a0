"""CPU: the variant matrix (tests/variant_matrix.py) names every kernel instantiation of csrc/launch_rule.h and no other, and a
word of the launch log (ac3mi_debug_launch_log) decodes to the name tests/launch_rule_c/main.cpp gives it."""
import ctypes
import re

import numpy as np

from tests import _harness as H
from tests import variant_matrix as V
from tests.test_launch_rule_cpu import program         # noqa: F401  (the fixture: main.cpp under -fsanitize=address,undefined)


def test_recipes_name_exactly_the_listed_variants(program):
    listed = program("lists").splitlines()
    assert len(listed) == len(set(listed)) == 79
    named = {k for r in V.RECIPES for k in r.chain}
    assert named == set(listed), (sorted(named - set(listed)), sorted(set(listed) - named))
    # a sibling route launches listed kernels too, and other ones than its recipe
    for r in V.RECIPES:
        for s in getattr(r, "siblings", ()):
            assert set(s.chain) <= set(listed), (r.name, s.what)
            assert s.chain != r.chain, (r.name, s.what)
    ids = [V.recipe_id(r) for r in V.RECIPES]
    assert len(ids) == len(set(ids))


def test_batch_shapes():
    """one-frame batches of 9 streams, multi-frame batches of 3 x 3: nothing else"""
    assert {r.shape for r in V.RECIPES} == {(9, 1), (3, 3)}


def test_log_words_decode_to_the_names_of_the_lists(program):
    """`words` prints family, word and name of the 79 variants in the order of `lists`, no (family, word) twice; the
    table the GPU tests decode with is that output, and an array as the tap fills it decodes to the names in order"""
    listed = program("lists").splitlines()
    rows = [line.split(" ", 2) for line in program("words").splitlines()]
    assert [r[2] for r in rows] == listed
    keys = [int(r[0]) << 24 | int(r[1]) for r in rows]
    assert len(set(keys)) == 79 and all(0 < int(r[0]) < 256 and 0 <= int(r[1]) < 1 << 24 for r in rows)
    table = V.word_table()
    assert table == dict(zip(keys, listed))
    # a family's name is the same in every row of it, and a plain kernel's word is 0
    fam = {}
    for r in rows:
        fam.setdefault(int(r[0]), set()).add(re.sub(r"<.*", "", r[2]))
    assert len(fam) == 10 and all(len(v) == 1 for v in fam.values())
    assert [r[1] for r in rows if r[2] in (V.LFSR, V.MANT)] == ["0", "0"]
    log = np.zeros(81, np.uint32)
    log[0], log[1:80] = 79, keys
    assert V.decode_log(log) == listed
    assert V.families([V.mdct(), V.packb(1, 1), V.MANT]) == {"enc_mdct_kernel", "enc_packb_kernel", "mant_kernel"}


def test_launch_log_refuses_bad_arguments():
    """ac3mi_debug_launch_log: AC3MI_ERR_ARG without a context, whatever the rest (no GPU needed to say so)"""
    lib = H.pkg().load_library()
    buf = (ctypes.c_uint32 * 4)()
    for log, cap in ((None, 0), (ctypes.cast(buf, ctypes.c_void_p), 4), (ctypes.cast(buf, ctypes.c_void_p), 0)):
        assert lib.ac3mi_debug_launch_log(None, log, cap) == -1
