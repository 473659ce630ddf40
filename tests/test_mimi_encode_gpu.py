"""HIP Mimi encoder (voice-clone prompts) against the third-party vectors and the oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAP_EPS = 1e-3  # a code may differ from the oracle's only where the oracle's two nearest rows are this close (squared distance)


def _state(seed):
    from smoltts_amd.codec.synthetic import synthetic_mimi_encoder_state, synthetic_mimi_state

    return {**synthetic_mimi_state(seed=seed), **synthetic_mimi_encoder_state(seed=seed)}


def _check_codes(got, want, orc, emb_ref, label):
    """A code may differ only where it happens: per frame (and per group: semantic, acoustic), the FIRST differing codebook must itself be an oracle near-tie (its two
    nearest rows within GAP_EPS at that codebook and frame); the codebooks behind it in that frame then legitimately differ (their
    residual is another one).  Returns the number of excused differing codes."""
    if np.array_equal(got, want):
        return 0
    gaps = orc.rvq_walk(emb_ref, torch.from_numpy(np.asarray(want))[None])["gap"][0].numpy()  # (nq, F), along the oracle's own codes
    for q0, f in {(min(q, 1), f) for q, f in np.argwhere(got != want)}:  # (the semantic codebook 0 and the acoustic group 1.. each
        q = q0 + int(np.argmax(got[q0:, f] != want[q0:, f])) if q0 else 0  # start from the latents: a residual chain of their own)
        assert gaps[q, f] < GAP_EPS, (f"{label}: frame {f} first differs at codebook {q} (code {got[q, f]}, oracle {want[q, f]}) where the "
                                      f"oracle's gap is {gaps[q, f]:.3e}, no near-tie (GAP_EPS {GAP_EPS:g})")
    return int((got != want).sum())


def test_encoder_reproduces_third_party_vectors(golden_dir):
    from oracle.mimi_oracle import MimiEncodeOracle
    from smoltts_amd.codec.synthetic import synthetic_pcm
    from smoltts_amd.engine import MimiEncoder

    g = np.load(golden_dir / "mimi_enc_hf.npz")
    st = _state(int(g["seed"]))
    for extra_right in (False, True):
        enc = MimiEncoder(st, 8, window=250, extra_right=extra_right)
        for L in g["lengths"].tolist():
            if L % 1920 and not extra_right:
                continue  # ragged lengths are pinned for the transformers padding convention only
            pcm = synthetic_pcm(L, int(g["pcm_seed"]))
            codes, emb, gap = enc.encode(pcm, return_aux=True)
            assert codes.shape == (8, enc.frames(L)) == g[f"codes_{L}"].shape[1:]
            ref = torch.from_numpy(g[f"emb_{L}"])[0].T  # (F, 512)
            err = float((emb.cpu() - ref).abs().max() / ref.abs().max())
            assert err < 1e-4, (L, extra_right, err)
            orc = MimiEncodeOracle(st, 8, window=250, extra_right=extra_right)
            _check_codes(codes.cpu().numpy(), g[f"codes_{L}"][0], orc, torch.from_numpy(g[f"emb_{L}"]), f"L={L}")
            assert float(gap.min()) > 0
        enc.close()


@pytest.mark.parametrize("L,window", [(1920 * 5 + 333, 0), (961, 0), (1, 0), (1920 * 21 - 1, 0), (1920 * 130, 250)])
def test_encoder_vs_oracle_reference_padding(L, window):
    """The reference's all-left padding (codec/conv.py:25-41) at ragged lengths, one sample, and beyond the
    250-position window (long signal: also the many-row GEMM path)."""
    from oracle.mimi_oracle import MimiEncodeOracle
    from smoltts_amd.codec.synthetic import synthetic_pcm
    from smoltts_amd.engine import MimiEncoder

    st = _state(5)
    pcm = synthetic_pcm(L, 4)
    enc = MimiEncoder(st, 8, window=window)
    codes, emb, gap = enc.encode(pcm, return_aux=True)
    orc = MimiEncodeOracle(st, 8, window=window)
    emb_ref = orc.embeddings(torch.from_numpy(pcm)[None, None])
    want = orc.rvq_encode(emb_ref)[0].numpy()
    assert codes.shape == want.shape
    err = float((emb.cpu() - emb_ref[0].T).abs().max() / emb_ref.abs().max())
    assert err < 1e-4, err
    flips = _check_codes(codes.cpu().numpy(), want, orc, emb_ref, f"L={L}")
    print(f"L={L}: {codes.shape[1]} frames, latent rel err {err:.2e}, {flips} near-tie flips, min gap {float(gap.min()):.3e}")
    # a second call reuses the workspace and must give the same answer (halos re-zeroed)
    assert torch.equal(enc.encode(pcm), codes)
    enc.close()


def test_encode_decode_round_trip_shapes_and_capacity():
    from smoltts_amd.codec.synthetic import synthetic_pcm
    from smoltts_amd.engine import MimiEncoder, MimiEngine, MimiSession, SmolttsError

    st = _state(2)
    enc = MimiEncoder(st, 8, max_positions=64)
    codes = enc.encode(synthetic_pcm(1920 * 8, 1))  # (8, 8)
    dec = MimiEngine(st, 8)
    sess = MimiSession(dec, max_batch=1, max_chunk_frames=8)
    pcm = sess.decode(codes.T.contiguous()[None])  # codes [B, F, nq] -> PCM
    assert pcm.shape == (1, 1920 * 8) and bool(torch.isfinite(pcm).all())
    with pytest.raises(SmolttsError, match="max_positions"):
        enc.encode(synthetic_pcm(960 * 65, 1))
    with pytest.raises(SmolttsError):
        enc.encode(np.zeros(0, np.float32))
    sess.close(); dec.close(); enc.close()
