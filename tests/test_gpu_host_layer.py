"""The Python layer that prepares a native call, on the device: the MLP descriptors of the inference path and of the training
Functions come from one field table (models.MLP_FIELD_TABLE), so they name the same storage slot for slot."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_inference_and_training_descriptors_share_every_slot():
    from hip_util import setup
    from pixel_nerf_multiscale_amd.model import models as M
    from pixel_nerf_multiscale_amd.render import autograd as ag
    fx, spec, net, rend = setup("tiny_ns2_codeview")
    read = lambda st, slots: [getattr(st, f) if b is None else getattr(st, f)[b] for f, b, _, _ in slots]
    for mlp in (net.mlp_coarse, net.mlp_fine):
        if mlp is None:
            continue
        ts = M.mlp_tensors(mlp)
        slots = M.mlp_slots(mlp.n_blocks, M.n_lin_z(mlp))
        hdr = ag._header(net, mlp, True)
        assert hdr["n_params"] == len(ts) == len(slots)
        m_inf, keep_inf = net.mlp_struct(mlp, "fp32")
        m_trn, keep_trn = ag._mlp_struct_from(hdr, ts)
        want = [t.data_ptr() for t in ts]                      # float32 contiguous parameters: the structs point at them
        assert len(set(want)) == len(want) and 0 not in want
        assert read(m_inf, slots) == read(m_trn, slots) == want
        assert [t.data_ptr() for t in keep_inf] == [t.data_ptr() for t in keep_trn] == want
        for name in ("d_in", "d_latent", "d_hidden", "d_out", "n_blocks", "combine_layer", "combine_type"):
            assert getattr(m_inf, name) == getattr(m_trn, name), name
        # gradients: slot i holds g_i, an absent gradient is NULL
        grads = [torch.zeros_like(t) if i % 5 else None for i, t in enumerate(ts)]
        g = ag._grads_struct_from(hdr, grads)
        assert read(g, slots) == [None if t is None else t.data_ptr() for t in grads]
