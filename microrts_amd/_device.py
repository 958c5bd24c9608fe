"""What DeviceVecEnv and ForwardModel share: a handle whose buffers are torch tensors in HBM and whose device calls
are ordered on torch's current HIP stream.  The GPU guard, the pointer and stream arguments of a ctypes call, and the
host-side state accessors, which wait for the stream before they read or write the handle."""
import ctypes

from ._packed import ptr


class DeviceHandle:
    _p = staticmethod(ptr)

    def _open(self, who, device):
        """torch and the device, or RuntimeError in the name of the class `who`: there is no CPU fallback.  Call first
        in __init__."""
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError(f"{who} needs an MI355X (torch.cuda is unavailable); there is no CPU fallback")
        self.torch = torch
        self.device = torch.device("cuda", device)
        return torch

    def _s(self, stream=None):
        if stream is None:  # torch's current stream, without building a Stream object per call
            return ctypes.c_void_p(self.torch._C._cuda_getCurrentRawStream(self.device.index))
        return ctypes.c_void_p(stream.cuda_stream)

    def synchronize(self):
        self.torch.cuda.current_stream(self.device).synchronize()

    def _host(self):
        """The handle, once the stream has run dry: the host-side accessors read and write it."""
        self.synchronize()
        return self._h

    def dump_state(self, slot):
        return self._host().dump(slot)

    def error_flags(self):
        return self._host().error_flags()

    def state_json(self, slot):
        """GameState.toJSON of the game behind `slot` (unit IDs = list positions)."""
        return self._host().state_json(slot)

    def set_state_json(self, slot, text):
        """GameState.fromJSON into the game behind `slot`."""
        self._host().set_state_json(slot, text)

    def close(self):
        self._host().close()
