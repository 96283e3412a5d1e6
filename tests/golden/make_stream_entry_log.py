"""Record the entry points every step of an eager SequenceRunner calls: tests/golden/stream_entry_log.json, [[names of step t]] for
the first four steps of tests/test_gpu_stream.py's stream (default precision).  Run it on the commit whose launch sequence is the
yardstick (it uses nothing that graph mode added), on a machine with a GPU:

    python -m tests.golden.make_stream_entry_log
"""
import json
import os

import torch

from magnet_amd import lib
from magnet_amd.sequence import SequenceRunner
from tests.test_gpu_stream import CAP, record_entry_log, stream_frames, stream_model

if __name__ == "__main__":
    lib.load()
    gpu = torch.device("cuda:0")
    log = record_entry_log(SequenceRunner(stream_model(gpu), CAP), stream_frames(gpu), gpu)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stream_entry_log.json")
    with open(path, "w") as fh:
        json.dump(log, fh, indent=0)
        fh.write("\n")
    print(path, [len(step) for step in log])
