"""Instance-ID maps: one frame's instance masks as ONE image whose pixel value says which instance owns the pixel
(LpfContext.set_masks_ids, lpf_set_masks_ids; LpfContext.run_wide, lpf_run_wide_ids).

Mask m is the set of pixels whose ID equals ``sel[m]``.  The compare is made on integers, never on 16 bits: a ``sel`` outside 0 .. 65535
matches no pixel of a uint16 map.  ``LPF_ID_NONE`` selects nothing, even in an int32 map that holds that value; it is what pads frames
with fewer instances than the batch's largest.  Equal entries are allowed: each gets its bit."""
import numpy as np

LPF_ID_NONE = -2 ** 31                  # include/lpf.h: a sel entry that selects nothing

_TORCH_IDS = {"torch.uint16": np.uint16, "torch.int32": np.int32}


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def id_dtype(ids):
    """np.uint16 or np.int32: the element type of a map (a NumPy array or a torch tensor); TypeError for anything else."""
    if _is_torch(ids):
        dt = _TORCH_IDS.get(str(ids.dtype))
    else:
        dt = {np.dtype(np.uint16): np.uint16, np.dtype(np.int32): np.int32}.get(getattr(ids, "dtype", None))
    if dt is None:
        raise TypeError("IdMasks: an ID map is uint16 or int32, got %s: convert with .astype(np.uint16) / .astype(np.int32) (torch: "
                        ".to(torch.int32)) -- int16 is refused because its sign is ambiguous, wider types because IDs above 2^31 - 1 "
                        "cannot be selected" % (getattr(ids, "dtype", type(ids).__name__),))
    return dt


def check_sel(sel, who="IdMasks"):
    """``sel`` as the library takes it: int32 [M].  ValueError for another shape, a non-integer dtype or a value outside int32."""
    s = np.asarray(sel if len(sel) else np.zeros(0, np.int32))
    if s.ndim != 1:
        raise ValueError("%s: sel must be a list of M integers, got shape %s" % (who, s.shape))
    if s.dtype.kind not in "iu":
        raise ValueError("%s: sel must hold integers, got %s" % (who, s.dtype))
    if len(s) and (int(s.min()) < -2 ** 31 or int(s.max()) > 2 ** 31 - 1):
        raise ValueError("%s: sel must lie within int32, got %d .. %d" % (who, int(s.min()), int(s.max())))
    return np.ascontiguousarray(s, dtype=np.int32)


class IdMasks:
    """One frame's masks as an instance-ID map: ``ids`` [H,W] uint16 or int32 (a NumPy array, or a torch tensor on the GPU), ``sel``
    int32 [M]; ``shape == (M, H, W)``.  Mask m = the pixels with ``ids == sel[m]``."""

    def __init__(self, ids, sel):
        self.id_dtype = id_dtype(ids)
        if len(ids.shape) != 2 or ids.shape[0] <= 0 or ids.shape[1] <= 0:
            raise ValueError("IdMasks: ids must be [H,W] with H, W > 0, got %s" % (tuple(ids.shape),))
        if _is_torch(ids) and not ids.is_cuda:
            raise ValueError("IdMasks: a torch map must be on the GPU (hand a host map over as a NumPy array)")
        self.ids = ids
        self.sel = check_sel(sel)
        self.shape = (len(self.sel), int(ids.shape[0]), int(ids.shape[1]))

    @property
    def on_device(self):
        return _is_torch(self.ids)

    @classmethod
    def from_instance_map(cls, ids, class_id=26, divisor=1000):
        """The instances of ONE class of a map whose pixel is ``semantic_id * divisor + instance_id``, the layout of KITTI-360's
        ``instance/`` images: ``sel`` = the ascending distinct IDs with ``id // divisor == class_id`` and ``id % divisor != 0`` (an
        instance ID of 0 marks pixels of the class that belong to no instance).  The distinct IDs are found on the host (np.unique); a
        GPU map is copied there for it.  ``class_id=26`` is believed to be ``car`` in KITTI-360's label table; it is a default, not a
        checked fact -- pass the class you mean."""
        id_dtype(ids)
        host = ids.cpu().numpy() if _is_torch(ids) else np.asarray(ids)
        u = np.unique(host).astype(np.int64)
        return cls(ids, u[(u // int(divisor) == int(class_id)) & (u % int(divisor) != 0)])

    def to_dense(self):
        """uint8 [M,H,W], 1 = member."""
        host = self.ids.cpu().numpy() if _is_torch(self.ids) else np.asarray(self.ids)
        sel = self.sel.astype(np.int64)
        member = (host.astype(np.int64)[None] == sel[:, None, None]) & (sel != LPF_ID_NONE)[:, None, None]
        return member.astype(np.uint8)

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, key):
        if not isinstance(key, slice):
            raise TypeError("IdMasks takes slices over masks (im[a:b]), got %r" % (key,))
        a, b, step = key.indices(self.shape[0])
        if step != 1:
            raise TypeError("IdMasks slices have step 1")
        return IdMasks(self.ids, self.sel[a:max(a, b)])      # (the map is shared, not copied)

    def __array__(self, *args, **kwargs):
        raise TypeError("IdMasks is not an array: use .to_dense() for entry points that take dense masks")

    def __repr__(self):
        return "IdMasks(M=%d, H=%d, W=%d, ids=%s%s)" % (self.shape + (np.dtype(self.id_dtype).name, ", on the GPU" if self.on_device else ""))
