"""Shared by the head-dim-128 tests: which launches keep their drop_p decisions in the keep-bit workspace once dh 128 exists, and the
engine step / fp64 oracle pair of test_dropout_step_gpu.py read out under that rule.

tests/dropout_refs.keepbit_path describes the launcher as it was with dh 32 and 64 only, and the tests written against it keep it as it
is.  A dh-128 model must be read out through this module: with the older rule its keep-bit sites would be taken for hash sites, and the
oracle would be fed masks the kernels never used."""
from unittest import mock

import dropout_refs as DR
import test_dropout_step_gpu as DS

# csrc/attention_long.hip at dh 128: image rows of 272 B, two 128-row chunk images and eight 32-row tiles (139,328 B with the flags),
# plus per padded key 4 B of bias - and, under CAUSAL / SEP, 4 B of second bias row, 1 B of mod_id and the tile / chunk votes
# (4 B per 32 and per 128 keys, 16 B) - within 160 KB.  The MASKED need is the larger one: 139,328 + 9.16 LkP <= 163,840 up to LkP = 2656.
DH128_MAX_LK = 2656


def keepbit_path(dh, Lq, Lk):
    """dropout_refs.keepbit_path, with dh 128: bit groups of 8 queries / keys and the LDS limit above."""
    if dh == 128:
        return Lq % 8 == 0 and Lk % 8 == 0 and Lk <= DH128_MAX_LK
    return DR.keepbit_path(dh, Lq, Lk)


def engine_step_and_oracle(*args, **kw):
    """test_dropout_step_gpu.engine_step_and_oracle with the step's masks collected under keepbit_path above."""
    with mock.patch.object(DR, "keepbit_path", keepbit_path):
        return DS.engine_step_and_oracle(*args, **kw)
