"""smirk_amd.losses without a GPU: every refusal of the three C entries (raw ctypes, dummy pointers: a refusal comes before anything touches the device, so
nothing is launched), the workspace query, the constants shared with the header, the host-side validation of the Python API, and the switch table of
FirstPathLoss against the trainer's own grouping (tests/loss_law.py total_law, smirk_trainer.py:134-154)."""
import ctypes as C
import itertools
import os
import re

import pytest
import torch

from loss_law import LOSS_KEYS, WEIGHTS_PRETRAIN, WEIGHTS_TRAIN, synth_first_path_inputs, total_law

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, ODD = C.c_void_p(0x10000), C.c_void_p(0x10004)                    # never dereferenced; ODD is not 16-byte aligned
BAD_ARG, WORKSPACE, UNSUPPORTED = -1, -2, -4


def _term(**kw):
    from smirk_amd import _lib as L
    t = L.SmirkLossTerm()
    a = dict(pred=P, target=P, row_flags=None, rows=4, row_stride=136, cols=34, kind=L.LOSS_SQUARE, C=0, HW=0, weight=1.0, loss_img=None, grad=None)
    a.update(kw)
    for k, v in a.items():
        setattr(t, k, v)
    return t


def _image(**kw):
    from smirk_amd import _lib as L
    a = dict(rows=2, C=3, HW=35, row_stride=105, cols=105, kind=L.LOSS_ABS_IMAGE)
    a.update(kw)
    return _term(**a)


def _arr(*terms):
    from smirk_amd import _lib as L
    return (L.SmirkLossTerm * len(terms))(*terms)


def _fwd(lib, terms, n=None, out_terms=P, out_total=P, ws=P, ws_bytes=None):
    n = len(terms) if n is None else n
    ws_bytes = max(lib.smirk_loss_workspace_bytes(terms, n), 256) if ws_bytes is None else ws_bytes
    return lib.smirk_loss_forward(terms, n, out_terms, out_total, ws, ws_bytes, None)


def _bwd(lib, terms, n=None, grad_total=P, ws=P, ws_bytes=None):
    n = len(terms) if n is None else n
    ws_bytes = max(lib.smirk_loss_workspace_bytes(terms, n), 256) if ws_bytes is None else ws_bytes
    return lib.smirk_loss_backward(terms, n, grad_total, ws, ws_bytes, None)


def test_c_entries_refuse_before_the_device_is_touched():
    from smirk_amd import _lib as L
    lib = L.lib()
    good = _arr(_term(), _image())
    for call in (_fwd, _bwd):
        assert call(lib, good, n=0) == BAD_ARG and call(lib, good, n=-1) == BAD_ARG
        assert call(lib, _arr(*[_term()] * (L.LOSS_MAX_TERMS + 1))) == BAD_ARG
        assert call(lib, None, n=1, ws_bytes=256) == BAD_ARG
        assert call(lib, good, ws=None) == BAD_ARG and call(lib, good, ws=ODD) == BAD_ARG
        assert call(lib, _arr(_term(pred=None))) == BAD_ARG
        for name in ("rows", "cols", "row_stride"):
            assert call(lib, _arr(_term(**{name: 0}))) == BAD_ARG, name
            assert call(lib, _arr(_term(**{name: -3}))) == BAD_ARG, name
        assert call(lib, _arr(_term(cols=137))) == BAD_ARG                                        # cols > row_stride
        assert call(lib, _arr(_term(kind=2))) == BAD_ARG and call(lib, _arr(_term(kind=-1))) == BAD_ARG
        assert call(lib, _arr(_image(C=0))) == BAD_ARG and call(lib, _arr(_image(HW=0))) == BAD_ARG
        assert call(lib, _arr(_image(C=-1))) == BAD_ARG and call(lib, _arr(_image(HW=-35))) == BAD_ARG
        assert call(lib, _arr(_image(row_stride=104, cols=104))) == BAD_ARG                       # C * HW is the row of an image term
        assert call(lib, _arr(_image(target=None))) == BAD_ARG and call(lib, _arr(_image(row_flags=P))) == BAD_ARG
        assert call(lib, _arr(_term(loss_img=P))) == BAD_ARG                                      # loss_img belongs to image terms
        for name in ("pred", "target", "grad"):
            assert call(lib, _arr(_term(**{name: ODD}))) == BAD_ARG, name
            assert call(lib, _arr(_image(**{name: ODD}))) == BAD_ARG, name
        assert call(lib, _arr(_image(loss_img=ODD))) == BAD_ARG
        assert call(lib, _arr(_term(), _term(rows=0))) == BAD_ARG                                 # every term is looked at, not the first alone
        # element counts that do not fit an int
        assert call(lib, _arr(_term(rows=1 << 20, row_stride=1 << 12, cols=1), ), ws_bytes=1 << 30) == UNSUPPORTED
        assert call(lib, _arr(_image(rows=1 << 16, C=1 << 4, HW=1 << 12, row_stride=1 << 16, cols=1 << 16)), ws_bytes=1 << 40) == UNSUPPORTED
        need = lib.smirk_loss_workspace_bytes(good, 2)
        assert call(lib, good, ws_bytes=need - 1) == WORKSPACE and call(lib, good, ws_bytes=0) == WORKSPACE
    assert _fwd(lib, good, out_terms=None) == BAD_ARG and _fwd(lib, good, out_total=None) == BAD_ARG
    assert _bwd(lib, good, grad_total=None) == BAD_ARG
    assert _bwd(lib, good) == 0                                                                   # no term asks for a gradient: nothing to launch, no error


def test_workspace_bytes_grow_with_the_terms():
    from smirk_amd import _lib as L
    lib, c = L.lib(), L.LOSS_CHUNK
    one = lambda t: lib.smirk_loss_workspace_bytes(_arr(t), 1)
    assert one(_term(rows=0)) == 0                                                                # a refused term has no workspace
    sizes = [one(_term(rows=r, row_stride=c, cols=c)) for r in (1, 2, 31, 32, 33, 64, 1000)]
    assert sizes == sorted(sizes) and sizes[0] >= 8 and sizes[-1] >= 8 * 1000 and sizes[-1] > sizes[0]
    sizes = [one(_term(rows=64, row_stride=4 * c, cols=k)) for k in (1, c - 1, c, c + 1, 4 * c)]
    assert sizes == sorted(sizes) and sizes[-1] >= 8 * 64 * 4
    sizes = [one(_image(rows=b, C=3, HW=224 * 224, row_stride=3 * 224 * 224, cols=3 * 224 * 224)) for b in (1, 2, 32, 64)]
    assert sizes == sorted(sizes) and sizes[-1] >= 8 * (64 * 224 * 224 // c)                      # one partial per chunk of pixels
    both = lib.smirk_loss_workspace_bytes(_arr(_term(rows=64, row_stride=c, cols=c), _image(rows=64, C=3, HW=c, row_stride=3 * c, cols=3 * c)), 2)
    assert both >= 8 * 128 and both >= one(_term(rows=64, row_stride=c, cols=c))
    # the layout depends on the shapes alone: a gradient pointer or a weight changes nothing
    assert one(_term(grad=P, weight=3.0)) == one(_term())


def test_constants_equal_the_header():
    from smirk_amd import _lib as L, losses
    hdr = open(os.path.join(REPO, "include", "smirk_hip.h")).read()
    val = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1))
    assert L.LOSS_CHUNK == losses.CHUNK == val("SMIRK_LOSS_CHUNK")
    assert L.LOSS_MAX_TERMS == losses.MAX_TERMS == val("SMIRK_LOSS_MAX_TERMS") >= 8
    assert (L.LOSS_SQUARE, L.LOSS_ABS_IMAGE) == (val("SMIRK_LOSS_SQUARE"), val("SMIRK_LOSS_ABS_IMAGE"))
    assert L.lib().smirk_abi_version() == L.ABI_VERSION
    fields = re.search(r"typedef struct SmirkLossTerm \{(.*?)\} SmirkLossTerm;", hdr, re.S).group(1)
    names = [n for decl in fields.split(";") for n in re.findall(r"[*\s,]([A-Za-z_]\w*)\s*(?=,|$)", decl.strip())]
    assert names == [n for n, _ in L.SmirkLossTerm._fields_], names
    assert C.sizeof(L.SmirkLossTerm) == 72


def test_python_api_validates_on_the_host():
    import smirk_amd
    from smirk_amd import FirstPathLoss, LossTerms, SmirkHipError, weighted_loss
    from smirk_amd.losses import Term, cycle_loss, effective_weights
    assert smirk_amd.losses.weighted_loss is weighted_loss and smirk_amd.first_path.first_path
    x, y = torch.rand(4, 136), torch.rand(4, 136)
    with pytest.raises(SmirkHipError, match="CPU"):
        weighted_loss([Term(x, y)])                                                               # CPU tensors: no fallback
    with pytest.raises(SmirkHipError, match="CPU"):
        cycle_loss(*[{k: torch.rand(2, n) for k, n in (("expression_params", 50), ("jaw_params", 3), ("eyelid_params", 2), ("shape_params", 300))}] * 2)
    with pytest.raises(SmirkHipError):
        weighted_loss([])
    with pytest.raises(SmirkHipError):
        weighted_loss([Term(x, y)] * 9)
    with pytest.raises(SmirkHipError):
        weighted_loss([Term(x, y, kind="huber")])
    enc, lf, lm, batch, recon, _ = synth_first_path_inputs(2, H=8, W=8)
    first = FirstPathLoss(WEIGHTS_TRAIN)
    with pytest.raises(SmirkHipError, match="CPU"):
        first(enc, lf, lm, batch, reconstructed_img=recon)
    with pytest.raises(SmirkHipError, match="unknown"):
        FirstPathLoss(dict(WEIGHTS_TRAIN, landmark_weight=1.0))                                   # an unknown weight key
    with pytest.raises(SmirkHipError, match="missing"):
        FirstPathLoss({k: v for k, v in WEIGHTS_TRAIN.items() if k != "jaw_regularization"})
    with pytest.raises(SmirkHipError, match="unknown"):
        first(enc, lf, lm, batch, extra={"style_loss": torch.zeros(())})
    with pytest.raises(SmirkHipError, match="scalar"):
        first(enc, lf, lm, batch, extra={"mica_loss": torch.zeros(2)})
    with pytest.raises(SmirkHipError, match="CPU"):
        first(enc, lf, lm, batch, extra={"mica_loss": torch.zeros(())})                           # checked up front, like every other operand
    assert effective_weights({k: v for k, v in WEIGHTS_TRAIN.items() if k != "cycle_loss"})["landmark_loss_mp"] == 100.0      # cycle_loss is not a first-path key
    t = LossTerms(("landmark_loss_fan", "landmark_loss_mp"), torch.tensor([0.25, 0.5]), zeros=("mica_loss",))
    assert t.as_dict() == {"landmark_loss_fan": 0.25, "landmark_loss_mp": 0.5, "mica_loss": 0} and t.loss_img is None


def test_python_api_validates_shapes_and_operands():
    """Shape and requires-grad refusals and the operands handed to the library, on host tensors that claim to be on the device: the validation looks at
    properties of the tensors only, so it runs to its end without a GPU."""
    from smirk_amd import SmirkHipError
    from smirk_amd import losses

    class Fake(torch.Tensor):
        """a CPU tensor that says it lives on the HIP device: lets the host-side validation run to its end without a device"""
        @property
        def is_cuda(self):
            return True

    fake = lambda t: t.as_subclass(Fake)
    x, y = fake(torch.rand(4, 136)), fake(torch.rand(4, 136))
    with pytest.raises(SmirkHipError, match="requires grad"):
        losses._prepare([losses.Term(x, fake(torch.rand(4, 136).requires_grad_(True)))])          # a target that requires grad
    with pytest.raises(SmirkHipError, match="does not match"):
        losses._prepare([losses.Term(x, fake(torch.rand(4, 135)))])
    with pytest.raises(SmirkHipError, match="cols"):
        losses._prepare([losses.Term(x, y, cols=137)])
    with pytest.raises(SmirkHipError, match="flags"):
        losses._prepare([losses.Term(x, y, flags=fake(torch.ones(3, dtype=torch.bool)))])
    with pytest.raises(SmirkHipError, match="flags must be"):
        losses._prepare([losses.Term(x, y, flags=fake(torch.ones(4)))])
    with pytest.raises(SmirkHipError, match="l1_image"):
        losses._prepare([losses.Term(x, y, kind="l1_image")])                                     # not [B, C, H, W]
    with pytest.raises(SmirkHipError, match="l1_image"):
        losses._prepare([losses.Term(fake(torch.rand(2, 3, 4, 4)), None, kind="l1_image")])       # no target
    with pytest.raises(SmirkHipError, match="loss_img"):
        losses._prepare([losses.Term(x, y, loss_img=True)])
    terms, ops = losses._prepare([losses.Term(x, y, flags=fake(torch.tensor([True, False, True, True])), cols=34),
                                  losses.Term(fake(torch.rand(8, 3, 5, 7)[1::4]), fake(torch.rand(2, 3, 5, 7)), kind="l1_image", loss_img=True)])
    assert ops[0][2].dtype == torch.uint8 and ops[0][2].tolist() == [1, 0, 1, 1]
    assert all(o.is_contiguous() and o.dtype == torch.float32 and o.data_ptr() % 16 == 0 for op in ops for o in op[:2])
    off = fake(torch.rand(4 * 136 + 1)[1:].view(4, 136))                                          # contiguous, but 4 bytes off a 16-byte boundary: copied
    assert off.data_ptr() % 16 == 4 and losses._prepare([losses.Term(off, fake(torch.rand(4, 136).double()))])[1][0][0].data_ptr() % 16 == 0
    arr = losses._structs(terms, ops, [None, None], [None, None])
    assert (arr[0].rows, arr[0].row_stride, arr[0].cols, arr[0].kind) == (4, 136, 34, 0)
    assert (arr[1].rows, arr[1].row_stride, arr[1].cols, arr[1].kind, arr[1].C, arr[1].HW) == (2, 105, 105, 1, 3, 35)


@pytest.mark.parametrize("switches", list(itertools.product((False, True), repeat=3)))
def test_first_path_switch_table_follows_the_trainer(switches):
    """smirk_trainer.py:134-154 on the weights alone: the factor each entry of `losses` has in loss_first_path, read off the trainer's own grouping by feeding it
    unit vectors, against the table FirstPathLoss applies, for every combination of optimize_shape, optimize_expression and enable_fuse_generator."""
    from smirk_amd import FirstPathLoss
    for w in (WEIGHTS_TRAIN, WEIGHTS_PRETRAIN, {k: float(i + 2) for i, k in enumerate(WEIGHTS_TRAIN)}):
        first = FirstPathLoss(w, *switches)
        assert first.enable_fuse_generator == switches[2] and set(first.weights) == set(LOSS_KEYS)
        for k in LOSS_KEYS:
            unit = {j: float(j == k) for j in LOSS_KEYS}
            assert first.weights[k] == float(total_law(unit, w, *switches)), (k, switches)
