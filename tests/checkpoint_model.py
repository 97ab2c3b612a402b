"""tests/handle_model.py's model of the handle, with one more event: the handle is saved to a checkpoint, closed, created again and loaded.  The sums, the counts, the
switches and the frame counter survive; what belonged to the handle that is gone does not: its snapshots (denoised, robust mean), its statistics, its bound buffer."""
from handle_model import HandleModel


class CheckpointedModel(HandleModel):
    def checkpoint_cycle(self):
        self.denoised = self.robust = None
        self.primary_rays = 0
        self.bound = False
        return ("ok", None)
