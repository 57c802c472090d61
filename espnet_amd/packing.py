"""Weight packs: a module's parameters in the layouts the kernels read, and when such a copy is (re)built.

A `Pack` owns the tensors it was built from and never changes once built: a caller that holds one may go on launching
kernels on its pointers whatever happens to the module meanwhile (a reload, a dtype switch, a rebuild for a longer
positional table).  `PackedModule.packed(device, pe_len)` returns the module's current pack when it satisfies the request
and otherwise builds a new one; `invalidate()` only drops the module's reference to it.

Builds are serialised by one process-wide lock (a lock per instance would make the modules unpicklable) with a check
before and after taking it, so host threads that ask for the same pack at once build it once; the common case, a current
pack, takes no lock.
"""
import itertools
import threading

import torch

from espnet_amd import lib as L

_BUILD_LOCK = threading.RLock()
_SERIALS = itertools.count(1)


class Pack:
    """One build of a module's kernel-layout weights.  `w` / `layers` are the module's C-ABI structs (if it has any), other
    named tensors are plain attributes; `serial` is unique in the process and identifies the build in cache keys."""

    def __init__(self, device: torch.device, dtype, act: torch.dtype, pe_len):
        self.device, self.dtype, self.act, self.pe_len = device, dtype, act, pe_len
        self.serial = next(_SERIALS)
        self.w = self.layers = None
        self.keep = []
        self._held = set()
        self._frozen = False

    def __setattr__(self, name, value):
        if self.__dict__.get("_frozen"):
            raise AttributeError(f"a pack does not change once built ({name})")
        object.__setattr__(self, name, value)

    def hold(self, t: torch.Tensor) -> torch.Tensor:
        """t on the pack's device as it is (dtype unchanged), owned by the pack."""
        t = t.to(self.device)
        self.keep.append(t)
        self._held.add(id(t))
        return t

    def A(self, t: torch.Tensor) -> torch.Tensor:
        """A matrix in the activation dtype."""
        return self.hold(t.detach().to(torch.float32).contiguous().to(self.act))

    def F(self, t: torch.Tensor) -> torch.Tensor:
        """An f32 vector or table."""
        return self.hold(t.detach().to(torch.float32).contiguous())

    def fill(self, struct, mapping: dict):
        """struct.<name> = the device address of each tensor of `mapping` (tensors this pack holds only)."""
        for k, t in mapping.items():
            if id(t) not in self._held:
                raise ValueError(f"{k}: a pointer of a pack must come from a tensor the pack holds")
            setattr(struct, k, t.data_ptr())


class PackedModule(torch.nn.Module):
    """Base of the modules whose weights the kernels read from a `Pack`.  A subclass implements `_build_pack(pk)` (fill `pk`
    through `pk.A` / `pk.F` / `pk.hold` / `pk.fill`) and may declare
      - `em_dtype`: the compute dtype the pack is built for (None: the layouts do not depend on it);
      - `pe_min`: the module has a positional table of `pk.pe_len` rows, built for max(pe_min, the longest request);
      - `_pack_current(pk)`: a further condition for the pack to be current (e.g. parameters of another module it copies)."""

    em_dtype = None
    pe_min = None
    _pack = None

    @property
    def act_dtype(self) -> torch.dtype:
        return torch.bfloat16 if self.em_dtype == L.EM_BF16 else torch.float32

    def _pack_current(self, pk: Pack) -> bool:
        return True

    def packed(self, device, pe_len: int = 0) -> Pack:
        """The current pack for `device` with a positional table of at least `pe_len` rows, built if needed."""
        pk = self._pack
        if (pk is not None and pk.device == device and pk.dtype == self.em_dtype and pk.pe_len >= pe_len
                and self._pack_current(pk)):
            return pk
        device = torch.device(device)
        with _BUILD_LOCK:
            pk = self._pack
            if (pk is not None and pk.device == device and pk.dtype == self.em_dtype and pk.pe_len >= pe_len
                    and self._pack_current(pk)):
                return pk
            rows = float("inf") if self.pe_min is None else max(self.pe_min, pe_len)
            pk = Pack(device, self.em_dtype, self.act_dtype, rows)
            self._build_pack(pk)
            if device.type == "cuda":  # (built on this thread's stream: complete before any other stream reads it)
                torch.cuda.current_stream(device).synchronize()
            pk._frozen = True
            self._pack = pk
            return pk

    def _build_pack(self, pk: Pack):
        raise NotImplementedError

    def invalidate(self):
        """Build a new pack at the next `packed()` call (packs already handed out stay valid)."""
        self._pack = None

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        r = super().load_state_dict(state_dict, strict=strict, **kw)
        self.invalidate()
        return r
