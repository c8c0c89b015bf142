"""The pipelined SOQPSK link's chain streams.

Under the library's default (WF_OPT_PIPE_RESERVE_CUS = -1, short bank) wf_link_run queues a block's whole chain — prologue,
front end, detector, fix-up, count — on ONE of two streams of the context, taken in turn.  What the single prologue stream
and the single back stream of the earlier form ordered for free is now an event edge each (the list stands where wf_link_run
sets the chains up): the next prologue behind this one (context-owned encoder scratch), the next back end behind this one (the
detector's proof records and repair lists), the chain behind the caller's stream.  None may move a count: the pipelined link
gives the sequential link's counts block for block.  Sizes: 4 000 symbols is under two detector waves, 65 600 one modulator
tile over 64, 300 001 several workgroups.
"""
import functools

import pytest

SPS = 8
NSYM = [4_000, 65_600, 300_001]
EBN0 = (4.0, 6.0, 10.0)


def _point(k, ebn0=None):
    """Block k's operating point and generator position: no two consecutive blocks alike."""
    return dict(ebn0_db=EBN0[k % 3] if ebn0 is None else ebn0, seed=5, stream_id=k, skip_bits=23 * k)


def _nine_blocks(link, ebn0=None):
    """9 blocks with a reset in the middle: both chains and both sets are reused several times.  Counts after every block."""
    got = []
    for k in range(9):
        if k == 4:
            link.reset_counts()
        link.run_block(**_point(k, ebn0))
        got.append(link.result())
    return got


@functools.lru_cache(maxsize=None)
def _sequential(nsym, warmup, ebn0):
    """The sequential link's (fuse 15) counts after each of the nine blocks, and the repairs it ran: computed once per shape."""
    from waveforms_amd import device as dev
    from waveforms_amd.link import SOQPSKLink

    seq = SOQPSKLink(nsym, SPS, fuse=15, warmup=warmup, private_ctx=True)
    dev.viterbi_repaired(reset=True, ctx=seq._ctx)
    want = _nine_blocks(seq, ebn0)
    repaired = dev.viterbi_repaired(reset=True, ctx=seq._ctx)
    del seq
    return tuple(want), repaired


def _streams():
    import torch

    return ((False, torch.cuda.current_stream()), (True, torch.cuda.Stream()))


@pytest.mark.gpu
@pytest.mark.parametrize("nsym", NSYM)
def test_chained_link_equals_the_sequential_link(nsym):
    """fuse 47 on a private context against fuse 15, block for block, from the NULL stream and from a stream of the caller's."""
    import torch

    from waveforms_amd import _hip
    from waveforms_amd.link import SOQPSKLink

    want, _ = _sequential(nsym, 0, None)
    assert want[-1][1] > 0
    for own, stream in _streams():
        with torch.cuda.stream(stream):
            pip = SOQPSKLink(nsym, SPS, fuse=47, private_ctx=True)
            assert _hip.get_option(pip._ctx, _hip.WF_OPT_PIPE_RESERVE_CUS) == -1 and pip.prologue_ahead
            assert tuple(_nine_blocks(pip)) == want, (nsym, own)
            del pip


@pytest.mark.gpu
@pytest.mark.parametrize("nsym", [65_600, 300_001])
def test_chained_link_with_the_generic_precoder_equals_the_sequential_link(nsym):
    """fuse bit 4: PRBS and precoder as the generic four launches, which work in the context's encoder scratch and table area —
    the one part of a prologue that consecutive chains share.  Alone, and in turn with a one-launch link on the shared context."""
    import torch

    from waveforms_amd.link import SOQPSKLink

    want, _ = _sequential(nsym, 0, None)
    for own, stream in _streams():
        with torch.cuda.stream(stream):
            pip = SOQPSKLink(nsym, SPS, fuse=63, private_ctx=True)
            assert pip.prologue_ahead
            assert tuple(_nine_blocks(pip)) == want, (nsym, own)
            del pip
            pair = [SOQPSKLink(nsym, SPS, fuse=fuse) for fuse in (63, 47, 63)]
            for k in range(4):
                for link in pair:
                    link.run_block(**_point(k))
            assert [link.result() for link in pair] == [want[3]] * 3, (nsym, own)
            del pair


@pytest.mark.gpu
@pytest.mark.parametrize("nsym", NSYM)
def test_chained_link_with_forced_repairs_equals_the_sequential_link(nsym):
    """A 2-row warm-up at 2 dB: nearly every chunk is repaired, so the fix-up of block k and the detector of block k + 1 both
    work through the context's one set of proof records and repair lists.  result() raises if a chunk is left unproven."""
    import torch

    from waveforms_amd import device as dev
    from waveforms_amd.link import SOQPSKLink

    want, seq_repaired = _sequential(nsym, 2, 2.0)
    assert want[-1][1] > 0 and seq_repaired > 0
    for own, stream in _streams():
        with torch.cuda.stream(stream):
            pip = SOQPSKLink(nsym, SPS, fuse=47, warmup=2, private_ctx=True)
            assert pip.prologue_ahead
            dev.viterbi_repaired(reset=True, ctx=pip._ctx)
            assert tuple(_nine_blocks(pip, 2.0)) == want, (nsym, own)
            assert dev.viterbi_repaired(reset=True, ctx=pip._ctx) > 0, (nsym, own)
            assert dev.viterbi_unmerged(reset=True, ctx=pip._ctx) == 0
            del pip


TURNS = ["AB" * 6, "AABB" * 3, "ABBA" * 3]


@pytest.mark.gpu
@pytest.mark.parametrize("turns", TURNS)
def test_two_chained_links_of_different_sizes_take_turns_on_one_context(turns):
    """4 000 and 300 001 symbols, both pipelined, on the SHARED per-device context: the short block's chain is through long
    before the long block's, so a missing edge would let a later block's prologue or back end overtake.  Each link equals its
    own sequential link after every round of turns."""
    import torch

    from waveforms_amd import _hip
    from waveforms_amd.link import SOQPSKLink

    sizes = {"A": 4_000, "B": 300_001}
    for own, stream in _streams():
        with torch.cuda.stream(stream):
            links = {(who, fuse): SOQPSKLink(n, SPS, fuse=fuse, private_ctx=fuse == 15) for who, n in sizes.items() for fuse in (15, 47)}
            assert links["A", 47]._ctx == links["B", 47]._ctx == _hip.ctx()
            assert links["A", 47].prologue_ahead and links["B", 47].prologue_ahead
            got = {k: [] for k in links}
            for fuse in (15, 47):
                blk = {"A": 0, "B": 0}
                for t, who in enumerate(turns):
                    links[who, fuse].run_block(**_point(blk[who]))
                    blk[who] += 1
                    if t % 4 == 3:
                        for w in sizes:
                            got[w, fuse].append(links[w, fuse].result())
            for who in sizes:
                assert got[who, 47] == got[who, 15], (who, turns, own)
                assert got[who, 15][-1][1] > 0
            del links


@pytest.mark.gpu
@pytest.mark.parametrize("private", [False, True])
def test_freeing_a_chained_link_leaves_nothing_pending(private):
    """A link is freed with its last blocks still queued and no synchronise of the caller's; a new link on the same context (the
    shared one, or — private — a fresh one where the old context's streams were destroyed with it) runs at once.  Counts are
    right, and the device and the context are clean afterwards."""
    import torch

    from waveforms_amd import _hip
    from waveforms_amd.link import SOQPSKLink

    nsym = 300_001
    want, _ = _sequential(nsym, 0, None)
    for own, stream in _streams():
        with torch.cuda.stream(stream):
            first = SOQPSKLink(nsym, SPS, fuse=47, private_ctx=private)
            for k in range(3):
                first.run_block(**_point(k))
            del first
            second = SOQPSKLink(nsym, SPS, fuse=47, private_ctx=private)
            for k in range(4):
                second.run_block(**_point(k))
            assert second.result() == want[3], (private, own)
            _hip.check(_hip.lib().wf_ctx_check(second._ctx, _hip.stream()))
            del second
            torch.cuda.synchronize()
