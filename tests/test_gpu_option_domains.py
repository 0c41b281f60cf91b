"""ia_set_option: every option accepts exactly its documented domain.

The domains below are written out from include/ia.h and from what ia_set_option accepted before it
had a table, not read from the library: the table is checked against an independent statement.
Only ia_set_option runs (no kernel is launched), on a context of this module's own, so nothing has
to be restored on the shared `ctx`.  The C ABI has no getter: that a refused call leaves the earlier
setting in force is read from Context.option(), which records a value only after the library
accepted it.
"""
import os
import re

import pytest
import torch  # noqa: F401  (before libia loads: torch's HIP runtime must be the process's first)

pytestmark = pytest.mark.gpu

FLAG = dict(good=(0, 1), bad=(-1, 2))
UPTO2 = dict(good=(0, 1, 2), bad=(-1, 3))
# name -> values accepted (the last one is left set: non-default where the domain has one) / refused
DOMAINS = dict(
    {n: FLAG for n in ('rec_wt', 'stamps', 'prune', 'shard_unpruned', 'k3p_blocks', 'fuse_gather', 'nn_bound',
                       'early_gather', 'gather_wave', 'prefetch_next', 'fuse_unpruned', 'pipeline_last',
                       'pipeline_record', 'xo_wait', 'xo_presort', 'matcher')},
    fuse_sort=UPTO2, exchange=UPTO2,
    k3p_variant=dict(good=(20, 21, 22, 24, 25), bad=(19, 23, 26, 0)),
    k3_variant=dict(good=(1,), bad=(0, 2)),
    row_source=dict(good=(0,), bad=(1, -1)),
    prune_group=dict(good=(1, 2, 4, 8), bad=(0, 3, 16)),
    shard_emulate=dict(good=(1, 64), bad=(0, 65)),
    prune_min_rows=dict(good=(1 << 19, 1), bad=(0, -1)),
    scan_wgs=dict(good=(8, 256, 128), bad=(0, 4, 12, 264)),
    time_dist=dict(good=(0, 1, 7), bad=()),
)
if 'IA_CU_SPLIT' not in os.environ:   # (with it the library refuses every stream_priority: no stream to recreate)
    DOMAINS['stream_priority'] = UPTO2
# flags whose library default is 1: the value left set before the refused calls is 0
DEFAULT_ON = ('rec_wt', 'prune', 'k3p_blocks', 'fuse_gather', 'nn_bound', 'early_gather', 'gather_wave', 'prefetch_next',
              'matcher')


@pytest.fixture(scope='module')
def dctx():
    from ia_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def _refused(dctx, name, value):
    from ia_amd import _native
    with pytest.raises(_native.IAError, match='IA_EINVAL'):
        dctx.set_option(name, value)


@pytest.mark.parametrize('name', sorted(DOMAINS))
def test_option_accepts_its_domain_and_nothing_else(dctx, name):
    good, bad = DOMAINS[name]['good'], DOMAINS[name]['bad']
    if name in DEFAULT_ON:
        good = good[::-1]
    for v in good:
        dctx.set_option(name, v)
    kept = good[-1]
    assert dctx.option(name) == kept
    for v in bad:
        _refused(dctx, name, v)
        assert dctx.option(name) == kept, 'a refused value replaced the setting'
    dctx.set_option(name, kept)   # and the option still takes a valid value afterwards


@pytest.mark.parametrize('name', ['no_such_option', 'prune ', '', 'Prune'])
def test_unknown_option_names_are_refused(dctx, name):
    _refused(dctx, name, 1)
    assert dctx.option(name) is None


def test_every_option_named_in_the_header_is_covered():
    """the option names quoted in include/ia.h's "Options:" comment are all in DOMAINS"""
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, '..', 'include', 'ia.h')).read()
    block = text[text.index('/* Options:'):text.index('int ia_set_option(')]
    named = set(re.findall(r'"([a-z0-9_]+)"', block))
    assert len(named) >= 24
    skipped = {'stream_priority'} - set(DOMAINS)
    assert named <= set(DOMAINS) | skipped, sorted(named - set(DOMAINS) - skipped)
