"""CPU: the host side of sequence inference (magnet_amd/sequence.py): the frame pool's bookkeeping, the slot table of a step and
what SequenceRunner refuses.  The pool's tensors are allocated on the CPU here; no kernel runs."""
import pytest
import torch

from magnet_amd.lib import MagnetError
from magnet_amd.magnet import MAGNET
from magnet_amd.sequence import FramePool, SequenceRunner, slot_table
from magnet_amd.standin import StubDNet, StubFNet, make_args


def _pool(capacity):
    return FramePool(capacity, 5, 7, 16, "bf16", "cpu")


def test_pool_layouts():
    p = _pool(3)
    assert tuple(p.feat.shape) == (3, 7, 9, 16) and p.feat.dtype == torch.bfloat16
    assert tuple(p.gmm.shape) == (3, 2, 5, 7) and p.gmm.dtype == torch.float32
    assert tuple(p.xd3_hi.shape) == tuple(p.xd3_lo.shape) == (3, 63, 256) and p.xd3_hi.dtype == p.xd3_lo.dtype == torch.bfloat16
    assert FramePool(1, 4, 4, 8, "fp32", "cpu").feat.dtype == torch.float32
    with pytest.raises(MagnetError):
        FramePool(2, 4, 4, 12, "fp32", "cpu")                      # F % 8


def test_slots_are_assigned_in_order_and_known_ids_are_kept():
    p = _pool(4)
    assert p.assign([("s", 0), ("s", 1), ("s", 0), ("s", 2)]) == [(0, 0), (1, 1), (3, 2)]       # (first position, slot)
    assert p.missing([("s", 2), ("s", 3), ("s", 3), None, ("s", 0)]) == [1]                     # only the unseen id, once
    assert p.assign([("s", 2), ("s", 3)]) == [(1, 3)]                                           # a known id is not assigned again
    assert p.slots([("s", 3), ("s", 0), None, ("s", 2)]) == [3, 0, -1, 2]
    assert len(p) == 4 and ("s", 1) in p and ("s", 9) not in p


def test_lru_eviction_order():
    p = _pool(3)
    p.assign(["a", "b", "c"])
    p.slots(["a"])                                                  # a is now the most recently used: b, c, a
    assert p.ids() == ["b", "c", "a"]
    assert p.assign(["d"]) == [(0, 1)]                              # b goes, d takes its slot
    assert "b" not in p and p.ids() == ["c", "a", "d"]
    assert p.assign(["e", "a"]) == [(0, 2)]                         # c goes
    assert p.ids() == ["d", "e", "a"]
    assert p.assign(["f"]) == [(0, 1)]                              # d goes
    assert p.slots(["e", "a", "f"]) == [2, 0, 1]


def test_a_frame_of_the_call_in_progress_survives_eviction():
    p = _pool(3)
    p.assign(["a", "b", "c"])                                       # a is the least recently used
    # the call names a (the oldest) together with two new frames: b and c must go, not a
    assert p.assign(["x", "a", "y"]) == [(0, 1), (2, 2)]
    assert p.slots(["a", "x", "y"]) == [0, 1, 2] and "b" not in p and "c" not in p


def test_capacity_below_one_calls_frames_raises():
    p = _pool(2)
    with pytest.raises(MagnetError, match="3 distinct frames"):
        p.assign(["a", "b", "a", "c"])
    assert len(p) == 0                                              # nothing was assigned
    assert p.assign(["a", "b", "a", None]) == [(0, 0), (1, 1)]      # repeats and "no frame" do not count


def test_unknown_id_raises_and_is_named():
    p = _pool(2)
    p.assign([("scene0", "4")])
    with pytest.raises(MagnetError, match=r"\('scene0', '5'\)"):
        p.slots([("scene0", "4"), ("scene0", "5")])
    p.assign(["u", "v"])                                            # evicts ('scene0', '4')
    with pytest.raises(MagnetError, match=r"\('scene0', '4'\)"):
        slot_table(p, ["u"], [("scene0", "4"), "v"])


def test_release_frees_the_slots_again():
    p = _pool(3)
    p.assign(["a", "b", "c"])
    p.release(["b", "zzz"])                                         # an id the pool does not hold is ignored
    assert "b" not in p and p.ids() == ["a", "c"]
    assert p.assign(["d"]) == [(0, 1)]                              # the freed slot goes out first, nothing is evicted
    assert p.slots(["a", "c", "d"]) == [0, 2, 1]


def test_folder_batches_has_the_length_the_sharded_loop_asks_for():
    from eval_synthetic import FolderBatches
    assert [len(FolderBatches(range(n), 2)) for n in (1, 4, 5)] == [1, 2, 3]


def test_slot_table_of_a_step():
    """B = 3 windows, V = 2 views, frames 0..4 walked with offsets -1 / +1: frame 2 is the reference of window 1, view 1 of window 0
    and view 0 of window 2.  Entry [b] is window b's reference, entry [B + v B + b] its view v."""
    p = _pool(8)
    p.assign([4, 3, 2, 1, 0])                                       # slots 0..4 in this order: frame f sits in slot 4 - f
    refs = [1, 2, 3]
    nghbrs = [0, 1, 2,                                              # view 0 (offset -1) of windows 0, 1, 2
              2, 3, 4]                                              # view 1 (offset +1)
    table = slot_table(p, refs, nghbrs)
    assert table == [3, 2, 1, 4, 3, 2, 2, 1, 0]
    B = 3
    assert table[1] == table[B + 1 * B + 0] == table[B + 0 * B + 2] == 2      # frame 2 in its three roles
    assert slot_table(p, refs, [0, 1, None, 2, 3, 4])[B + 2] == -1             # a missing neighbour
    with pytest.raises(MagnetError, match="view-major"):
        slot_table(p, refs, nghbrs[:5])
    with pytest.raises(MagnetError, match="reference"):
        slot_table(p, [1, None, 3], nghbrs)


def _model(**kw):
    args = make_args(D=8, iters=1, dpv_h=8, dpv_w=8)
    args.downsample_ratio = kw.pop("ratio", 4)
    return MAGNET(args, d_net=StubDNet(1), f_net=StubFNet(2, fdim=16), **kw)


def test_runner_refuses_what_is_not_the_matrix_core_inference_path():
    with pytest.raises(MagnetError, match="conv_backend='mfma'"):
        SequenceRunner(_model(conv_backend="torch"), 4)
    with pytest.raises(MagnetError, match="downsample_ratio 4"):
        SequenceRunner(_model(ratio=8), 4)
    with pytest.raises(MagnetError, match="capacity"):
        SequenceRunner(_model(), 0)
    r = SequenceRunner(_model(), 4)
    with pytest.raises(MagnetError, match="inference"):            # grad enabled with trainable heads
        r.add(["a"], torch.zeros(1, 3, 32, 32))
    with torch.no_grad():
        with pytest.raises(MagnetError, match="no CPU fallback"):
            r.add(["a"], torch.zeros(1, 3, 32, 32))
        with pytest.raises(MagnetError, match=r"'a'"):             # refine before anything was added names the frame
            r.refine(["a"], ["b", "c"], None, None, None)
        with pytest.raises(MagnetError, match="2 frame ids for 1 images"):
            r.add(["a", "b"], torch.zeros(1, 3, 32, 32))
    r.pool = FramePool(4, 8, 8, 16, "fp32", "cpu")
    r.pool.assign(["a", "b"])
    with torch.no_grad():
        with pytest.raises(MagnetError, match=r"'c'"):
            r.refine(["a"], ["b", "c"], None, None, None)
        with pytest.raises(MagnetError, match="5 distinct frames"):
            r.add(list("abcde"), torch.zeros(5, 3, 32, 32))
