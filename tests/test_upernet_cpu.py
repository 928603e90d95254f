"""UperNet-Swin without a GPU: the native tensor table against transformers' state dict (keys, order, shapes, dtypes), the
transformers-4.x key names of the reference's checkpoints through checkpoint.load_model, the HuggingFace factory branch and the
refusals.  The model's arithmetic is tested on the GPU (tests/test_gpu_upernet.py)."""
import re

import pytest
import torch

SMALL, TINY = (2, 2, 18, 2), (2, 2, 6, 2)


def library_model(num_channels=3, num_labels=19, depths=SMALL):
    from transformers import SwinConfig, UperNetConfig, UperNetForSemanticSegmentation
    torch.manual_seed(0)
    bc = SwinConfig(embed_dim=96, depths=list(depths), num_heads=[3, 6, 12, 24], window_size=7, num_channels=num_channels,
                    out_features=["stage1", "stage2", "stage3", "stage4"])
    cfg = UperNetConfig(backbone_config=bc, hidden_size=512, pool_scales=[1, 2, 3, 6], use_auxiliary_head=True, auxiliary_in_channels=384,
                        auxiliary_channels=256, auxiliary_num_convs=1, num_labels=num_labels)
    return UperNetForSemanticSegmentation(cfg).eval()


@pytest.mark.parametrize("depths,channels,entries,params", [(TINY, 3, 309, 59842528), (SMALL, 3, 513, 81160432),
                                                            (TINY, 5, 309, None), (SMALL, 5, 513, None)])
def test_state_dict_is_the_librarys(depths, channels, entries, params):
    import flair_amd
    ref = library_model(channels, 19, depths).state_dict()
    m = flair_amd.UperNetForSemanticSegmentation(num_channels=channels, num_labels=19, depths=depths)
    sd = m.state_dict()
    assert list(sd) == list(ref) and len(sd) == entries
    for k, v in ref.items():
        assert sd[k].shape == v.shape and sd[k].dtype == v.dtype, k
    if params is not None:
        assert sum(p.numel() for p in m.parameters()) == params
    m.load_state_dict(ref, strict=True)
    got = m.state_dict()
    assert all(torch.equal(got[k], v) for k, v in ref.items())


# the transformers-4.x names (the reference pins transformers <= 4.50.3): the rename table read backwards
_TO_LEGACY = (
    (r"^backbone\.swin\.embeddings\.", "backbone.embeddings."),
    (r"^backbone\.swin\.encoder\.", "backbone.encoder."),
    (r"attention\.q_proj\.", "attention.self.query."),
    (r"attention\.k_proj\.", "attention.self.key."),
    (r"attention\.v_proj\.", "attention.self.value."),
    (r"attention\.relative_position_bias\.relative_position_bias_table", "attention.self.relative_position_bias_table"),
    (r"attention\.o_proj\.", "attention.output.dense."),
    (r"mlp\.fc1\.", "intermediate.dense."),
    (r"mlp\.fc2\.", "output.dense."),
)


def _legacy(sd):
    out = {}
    for k, v in sd.items():
        if k.startswith("backbone.swin.layernorm."):   # 4.x SwinBackbone had no final norm (5.x wraps a whole SwinModel)
            continue
        for pat, rep in _TO_LEGACY:
            k = re.sub(pat, rep, k)
        out[k] = v
        if k.endswith("attention.self.relative_position_bias_table"):
            out[k.replace("relative_position_bias_table", "relative_position_index")] = torch.zeros(49 * 49, dtype=torch.int64)
    return out


def test_legacy_checkpoint_loads_through_load_model(tmp_path):
    """A Lightning .ckpt with the 4.x names (model.seg_model. prefix, a criterion.weight entry, the relative_position_index
    buffers 4.x saved, no backbone.swin.layernorm) loads strictly through checkpoint.load_model and gives the library's tensors."""
    from flair_amd import checkpoint
    ref = library_model(3, 19, TINY).state_dict()
    legacy = _legacy(ref)
    assert "backbone.encoder.layers.0.blocks.1.output.dense.weight" in legacy
    assert "backbone.encoder.layers.0.blocks.1.attention.output.dense.weight" in legacy
    assert not any("q_proj" in k or "swin." in k for k in legacy)
    sd = {"model.seg_model." + k: v for k, v in legacy.items()}
    sd["criterion.weight"] = torch.ones(19)
    path = tmp_path / "upernet_swin_tiny.ckpt"
    torch.save({"epoch": 3, "global_step": 30, "state_dict": sd}, path)
    config = {"model_framework": {"model_provider": "HuggingFace", "HuggingFace": {"org_model": "openmmlab/upernet-swin-tiny"}},
              "use_metadata": False, "channels": [1, 2, 3], "classes": {i: [1, str(i)] for i in range(1, 20)},
              "model_weights": str(path)}
    model = checkpoint.load_model(config)
    got = model.state_dict()
    assert list(got) == list(ref)
    assert all(torch.equal(got[k], v) for k, v in ref.items())


def test_factory_builds_three_band_upernet_and_refuses_others():
    import flair_amd
    cfg = {"model_framework": {"model_provider": "HuggingFace", "HuggingFace": {"org_model": "openmmlab/upernet-swin-small"}},
           "use_metadata": False, "channels": [1, 2, 3], "classes": {i: [1, str(i)] for i in range(1, 20)}}
    f = flair_amd.FLAIR_ModelFactory(cfg)
    assert isinstance(f.seg_model, flair_amd.UperNetForSemanticSegmentation)
    assert f.seg_model.num_labels == 19 and f.seg_model.config.depths == SMALL and f.seg_model.num_channels == 3
    with pytest.raises(NotImplementedError, match="num_channels"):
        flair_amd.FLAIR_ModelFactory({**cfg, "channels": [1, 2, 3, 4, 5]})
    tiny = {**cfg, "model_framework": {"model_provider": "HuggingFace", "HuggingFace": {"org_model": "openmmlab/upernet-swin-tiny"}}}
    assert flair_amd.FLAIR_ModelFactory(tiny).seg_model.config.depths == TINY
    seg = {**cfg, "channels": [1, 2, 3, 4, 5],
           "model_framework": {"model_provider": "HuggingFace", "HuggingFace": {"org_model": "nvidia/mit-b2"}}}
    assert isinstance(flair_amd.FLAIR_ModelFactory(seg).seg_model, flair_amd.SegformerForSemanticSegmentation)


def test_refusals():
    import flair_amd
    from flair_amd.upernet import config_for_upernet
    for name in ("openmmlab/upernet-swin-base", "openmmlab/upernet-convnext-small", "openmmlab/upernet-swin-large"):
        with pytest.raises(NotImplementedError):
            config_for_upernet(name)
    with pytest.raises(ValueError, match="7 x 7"):
        flair_amd.UperNetForSemanticSegmentation(num_labels=19, window_size=12)
    with pytest.raises(RuntimeError):
        flair_amd.UperNetForSemanticSegmentation(num_labels=19).train()
