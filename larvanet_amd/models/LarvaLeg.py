"""LarvaNet with early-exit inference: drop-in for the reference plugin models/LarvaLeg.py.

Same network and checkpoints as LarvaNet; `--leg=k` makes forward() stop after body k-1 and
return that body's exit (k = num_modules is the full network, k = 0 returns the bicubic base
image alone) -- models/LarvaLeg.py:52, 275, 289-300.  Training is unchanged (all exits).

The early-exit pieces are shared with LarvaLegV2: EarlyExitRoute on the module, EarlyExitFlags on the plugin."""
from . import LarvaNet as V1
from . import LarvaNetV2 as V2


def create_model():
    return LarvaNet()


class EarlyExitRoute:
    """`--leg=k` on a LarvaNetModule (V1 or V2): the inference route stops after body k-1 at that body's exit."""

    def __init__(self, args):
        super().__init__(args)
        self.leg = args.leg
        if not 0 <= self.leg <= self.len:
            raise ValueError("--leg must be in [0, num_modules]")

    def route(self):
        return self.leg, (getattr(self, "body_%d" % (self.leg - 1)).leg if self.leg else None)


class EarlyExitFlags:
    """The plugin side of `--leg`: the flag itself and the halo of the shortened route."""

    has_cooldown = False   # (V2's flag set)
    tail_on_inference_route = False   # (LarvaLegV2: the V2 tail is trained, never on the --leg route)

    def _add_args(self, parser):
        # flag set and defaults of models/LarvaLeg.py:46-61 and models/LarvaLegV2.py:46-61 (= LarvaNetV2's plus --leg)
        V2.LarvaNet._add_args(self, parser)
        parser.add_argument("--leg", type=int, default=4, help="The early exit leg number, starts at 1.")

    def receptive_halo(self):
        k = self.args.leg
        return 2 if k == 0 else 1 + 2 * sum(V1.parse_num_blocks(self.args)[:k]) + 2


class LarvaNetModule(EarlyExitRoute, V1.LarvaNetModule):
    pass


class LarvaNet(EarlyExitFlags, V1.LarvaNet):
    module_class = LarvaNetModule
