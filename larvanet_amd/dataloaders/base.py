"""The data-loader plugin contract of the reference (dataloaders/base.py:9-111), restated.
Images travel as numpy CHW arrays on the 0-255 scale (float32 for training patches, uint8 for
validation images); nothing is normalised anywhere."""


def create_loader():
    return BaseLoader()


class SeededStream:
    """sampler_state() / load_sampler_state() of a loader whose every draw comes from ONE RandomState, `self.rng`, seeded
    from --data_seed: the state is that generator's.  Without a seed the stream is fresh entropy per process and there
    is nothing to continue: None."""

    def sampler_state(self):
        if getattr(self.args, "data_seed", None) is None:
            return None
        return self.rng.get_state()

    def load_sampler_state(self, state):
        self.rng.set_state(state)


class BaseLoader:
    def __init__(self):
        self.is_threaded = False

    def parse_args(self, args):
        """Consume known flags from `args`; returns (Namespace copy, leftover list)."""
        raise NotImplementedError

    def prepare(self, scales):
        raise NotImplementedError

    def get_num_images(self):
        raise NotImplementedError

    def get_patch_batch(self, batch_size, scale, input_patch_size):
        """-> (list of LR patches, list of HR patches)"""
        raise NotImplementedError

    def get_random_image_patch_pair(self, scale, input_patch_size):
        raise NotImplementedError

    def get_image_patch_pair(self, image_index, scale, input_patch_size):
        raise NotImplementedError

    def get_image_pair(self, image_index, scale):
        """-> (LR image, HR image, image name)"""
        raise NotImplementedError

    def get_truth_image(self, image_index, scale):
        """-> (HR image, image name) without touching the LR image where a loader can (device_patch_loader
        --lr_from_hr makes the LR images itself)."""
        _, hr, name = self.get_image_pair(image_index, scale)
        return hr, name

    # a training state (models/LarvaNet.save_training_state) continues the patch stream through these two
    def sampler_state(self):
        """The sampler's position in its random stream as a picklable object, or None when this loader cannot be
        continued (threads that prefetch, a stream that was never seeded)."""
        return None

    def load_sampler_state(self, state):
        """Continue the stream from a sampler_state() of a loader prepared with the same flags."""
        raise NotImplementedError("%s cannot continue a patch stream" % type(self).__name__)

    # threaded loaders only
    def start_training_queue_runner(self, batch_size, input_patch_size):
        raise NotImplementedError

    def stop_queue_runners(self):
        raise NotImplementedError

    def get_queue_data(self, scale):
        raise NotImplementedError
