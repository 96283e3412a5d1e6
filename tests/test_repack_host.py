"""The repack rule of the four weight-packing runners, on the CPU: packed() is cached, and an in-place change of a tensor it was built
from (an optimizer step, load_state_dict, a BatchNorm update: data_ptr stays, _version moves) gives new planes."""
import pytest
import torch
import torch.nn as nn

from magnet_amd.convnet import ConvStackMFMA
from magnet_amd.dnet import DenseDepthDecoder, DNetMFMA
from magnet_amd.fnet import FNET, FNetMFMA
from magnet_amd.train_fnet import FNetTrainHIP

CPU = torch.device("cpu")


def _stack():
    seq = nn.Sequential(nn.Conv2d(40, 128, 3, padding=1), nn.ReLU(), nn.Conv2d(128, 128, 1), nn.ReLU(), nn.Conv2d(128, 128, 1), nn.ReLU(),
                        nn.Conv2d(128, 2, 1))
    return ConvStackMFMA(seq), seq[0].weight, None, lambda P: P[0]["w_hi"]


def _psm(runner):
    psm = FNET(type("A", (), {"FNET_architecture": "PSM-Net", "FNET_feature_dim": 32})()).f_net.eval()
    bn = psm.layer1[0].conv1[0][1]
    return runner(psm), psm.layer1[0].conv1[0][0].weight, bn.running_var, lambda P: P["layer1.0.conv1"][0]


def _dnet():
    dec = DenseDepthDecoder(dnet=True).eval()
    return DNetMFMA(dec), dec.up3._net[3].weight, dec.up3._net[4].running_var, lambda P: P["up3.1"][0]


CASES = {"ConvStackMFMA": (_stack, None), "FNetMFMA": (lambda: _psm(FNetMFMA), True), "FNetTrainHIP": (lambda: _psm(FNetTrainHIP), False),
         "DNetMFMA": (_dnet, True)}


@pytest.mark.parametrize("name", list(CASES))
def test_packed_is_cached_and_follows_in_place_changes(name):
    make, stat_repacks = CASES[name]
    runner, weight, stat, plane = make()
    P = runner.packed(CPU)
    assert runner.packed(CPU) is P                                                       # cached
    old = plane(P).clone()
    if name == "ConvStackMFMA":
        split, chain = runner.packed_first_split(CPU, 8, 32), runner._chain
        assert runner.packed_first_split(CPU, 8, 32) is split and chain is not None
    with torch.no_grad():
        weight.mul_(2)                                                                   # as an optimizer step: in place
    P2 = runner.packed(CPU)
    assert P2 is not P and runner.packed(CPU) is P2
    assert not torch.equal(plane(P2), old)
    if name == "ConvStackMFMA":
        split2 = runner.packed_first_split(CPU, 8, 32)
        assert split2 is not split and not torch.equal(split2[0]["w_hi"], split[0]["w_hi"])
        assert runner._chain is not chain and torch.equal(runner._chain["w_hi"], chain["w_hi"])   # rebuilt; the 1x1 layers did not change
        with torch.no_grad():
            runner.layers[1][0].weight.mul_(2)
        runner.packed(CPU)
        assert not torch.equal(runner._chain["w_hi"], chain["w_hi"])
        return
    old = plane(P2).clone()
    stat.mul_(4)                                                                         # a BatchNorm running statistic, in place
    P3 = runner.packed(CPU)
    if stat_repacks:                                                                     # eval-mode runners fold the statistics in
        assert P3 is not P2 and not torch.equal(plane(P3), old)
    else:                                                                                # the training forward reads batch statistics
        assert P3 is P2
