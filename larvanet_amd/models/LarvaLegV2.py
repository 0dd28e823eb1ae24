"""LarvaNetV2 with early-exit inference: drop-in for the reference plugin models/LarvaLegV2.py.

The V2 network and its checkpoints (tail.* keys included; training is V2's: every exit plus the tail,
models/LarvaLegV2.py:102-124), but forward() stops after body k-1 and returns that body's exit for `--leg=k`
(k = 0: the bicubic base image alone) -- the tail is not evaluated (models/LarvaLegV2.py:52, 342, 358-367)."""
from . import LarvaNetV2 as V2
from .LarvaLeg import EarlyExitFlags, EarlyExitRoute


def create_model():
    return LarvaNet()


class LarvaNetModule(EarlyExitRoute, V2.LarvaNetModule):
    pass


class LarvaNet(EarlyExitFlags, V2.LarvaNet):
    # EarlyExitFlags comes first in the bases: its tail_on_inference_route = False is the one V2.LarvaNet.prepare() reads
    # here, so more than 8 bodies are refused for training only (the --leg route never reaches the tail's merge conv)
    module_class = LarvaNetModule
