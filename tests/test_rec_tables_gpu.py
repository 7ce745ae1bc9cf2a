"""GPU tests of the .rec coder under empirical symbol tables (csrc/irec_rec.hip, csrc/irec_rec_tables.hip): the device entry points against the files of
the reference-shaped Python writer, the host entry points and the core's host hooks (tests/rec_tables_cases.py: every file the device
sees here has been through the same lane functions on a CPU first, and every table was made by irec_rec_tables_build), two calls in
flight on two streams, the histogram kernel against its host twin, and the two models from fitted tables to pixels.  Every comparison
is byte, integer or torch.equal."""
import functools

import numpy as np
import pytest
import torch

import rec_tables_cases as C

pytestmark = pytest.mark.gpu

CASES = range(len(C.case_names()))


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                            # (a copy: the cases are read-only)


@pytest.mark.parametrize("which", CASES, ids=C.case_names())
def test_device_files_equal_the_python_writer_and_the_host(engine, which):
    from irec.io import utils as U
    c = C.cases()[which]
    n, total = c["K"].shape[0], int(c["offsets"][-1])
    both = _dev(C.joined(c["K"], c["idx"])).view(n, -1, 1 + C.MAX_K)
    for K, idx in ((_dev(c["K"]), _dev(c["idx"])), (both[..., 0], both[..., 1:])):          # the packed and the joined-tensor strides
        blob, off = U.encode_files_device_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, K, idx, c["max_index"], c["bpr"], tables=c["tables"])
        assert np.array_equal(off.cpu().numpy(), c["offsets"]) and np.array_equal(blob.cpu().numpy(), c["blob"])
    out = torch.full((total + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    off, status, _ = U._encode_files_device_ragged_launch(C.SEED, C.SHAPE, C.BLOCK_SIZE, _dev(c["K"]), _dev(c["idx"]), c["max_index"], c["bpr"],
                                                          out[:total], c["tables"])         # exactly enough room
    assert np.array_equal(out[:total].cpu().numpy(), c["blob"]) and (out[total:] == 0xAB).all() and not status.any()
    out.fill_(0xAB)
    off, status, _ = U._encode_files_device_ragged_launch(C.SEED, C.SHAPE, C.BLOCK_SIZE, _dev(c["K"]), _dev(c["idx"]), c["max_index"], c["bpr"],
                                                          out[:total - 1], c["tables"])     # one byte short: the size, and nothing written
    assert int(off[-1]) == total and (out == 0xAB).all() and not status.any()
    host_blob, host_off = U.encode_files_ragged(C.SEED, C.SHAPE, C.BLOCK_SIZE, c["K"], c["idx"], c["max_index"], c["bpr"], tables=c["tables"])
    core, core_off, core_status = C.core_encode(c["K"], c["idx"], c["max_index"], c["bpr"], C.raw_tables(c["tables"]), total)
    assert np.array_equal(host_blob, c["blob"]) and np.array_equal(core[:total], c["blob"]) and np.array_equal(core_off, host_off)
    hdr, K2, idx2 = U.decode_files_device_ragged(_dev(c["blob"]), c["offsets"], c["bpr"], C.MAX_K, tables=c["tables"])
    hdr_c, K_c, idx_c, _ = C.core_decode(c["blob"], c["offsets"], c["bpr"], C.MAX_K, C.raw_tables(c["tables"]))
    assert np.array_equal(K2.cpu().numpy(), c["K"]) and np.array_equal(idx2.cpu().numpy(), c["idx_zeroed"])
    assert np.array_equal(hdr.cpu().numpy(), hdr_c.astype(np.int64)) and np.array_equal(K_c, c["K"]) and np.array_equal(idx_c, c["idx_zeroed"])


def test_uniform_forms_take_tables_and_errors_name_the_image(engine):
    from irec.io import utils as U
    c = C.cases()[C.case_names().index("3x3_3-both")]
    K3, idx3 = _dev(c["K"]).view(3, 2, 3), _dev(c["idx"]).view(3, 2, 3, C.MAX_K)
    blob, off = U.encode_files_device(C.SEED, C.SHAPE, C.BLOCK_SIZE, K3, idx3, c["max_index"], tables=c["tables"])
    assert np.array_equal(blob.cpu().numpy(), c["blob"]) and np.array_equal(off.cpu().numpy(), c["offsets"])
    hdr, K, idx = U.decode_files_device(blob, off, 2, 3, C.MAX_K, tables=c["tables"])
    assert K.shape == (3, 2, 3) and torch.equal(K, K3) and np.array_equal(idx.cpu().numpy().reshape(3, 6, -1), c["idx_zeroed"])
    with pytest.raises(ValueError, match=r"empirical count tables.*\(image 0\)"):
        U.decode_files_device(blob, off, 2, 3, C.MAX_K)
    bad = idx3.clone()
    bad[1, 0, 0, 0] = 20
    Kb = K3.clone()
    Kb[1, 0, 0] = 1
    with pytest.raises(ValueError, match=r"index does not fit.*\(image 1\)"):
        U.encode_files_device(C.SEED, C.SHAPE, C.BLOCK_SIZE, Kb, bad, c["max_index"], tables=c["tables"])


def test_device_reader_equals_the_core_on_damaged_flagged_files(engine):
    from irec.io import utils as U
    d = C.damaged_set()
    hdr_c, K_c, idx_c, status_c = C.core_decode(d["blob"], d["offsets"], C.DAMAGED_BPR, C.DAMAGED_MK, C.raw_tables(d["tables"]))
    hdr, K, idx, status = U._decode_files_device_ragged_launch(_dev(d["blob"]), d["offsets"], C.DAMAGED_BPR, C.DAMAGED_MK, tables=d["tables"])
    assert np.array_equal(status.cpu().numpy(), status_c) and np.array_equal(status_c == 0, d["ok"])
    assert np.array_equal(hdr.cpu().numpy().view(np.uint32), hdr_c) and np.array_equal(K.cpu().numpy(), K_c) and np.array_equal(idx.cpu().numpy(), idx_c)


def test_two_calls_in_flight_on_two_streams_with_different_tables(engine):
    from irec.io import utils as U
    a = C.cases()[C.case_names().index("70x2_2_2-both")]
    b = C.cases()[C.case_names().index("3x3_3-index-lds")]
    ins = {id(c): (_dev(c["K"]), _dev(c["idx"]), torch.empty(int(c["offsets"][-1]), dtype=torch.uint8, device="cuda"), c["tables"].to("cuda"))
           for c in (a, b)}
    torch.cuda.synchronize()
    streams, outs = [torch.cuda.Stream(), torch.cuda.Stream()], {}
    for _ in range(3):
        for c, s in ((a, streams[0]), (b, streams[1])):
            K, idx, out, _ = ins[id(c)]
            with torch.cuda.stream(s):
                off, status, _ = U._encode_files_device_ragged_launch(C.SEED, C.SHAPE, C.BLOCK_SIZE, K, idx, c["max_index"], c["bpr"], out, c["tables"])
                outs[id(c)] = (off, status, U._decode_files_device_ragged_launch(out, off, c["bpr"], C.MAX_K, on_device=True, tables=c["tables"]))
    torch.cuda.synchronize()
    for c in (a, b):
        off, status, (hdr, K2, idx2, st2) = outs[id(c)]
        assert np.array_equal(ins[id(c)][2].cpu().numpy(), c["blob"]) and np.array_equal(off.cpu().numpy(), c["offsets"])
        assert not status.any() and not st2.any() and np.array_equal(K2.cpu().numpy(), c["K"]) and np.array_equal(idx2.cpu().numpy(), c["idx_zeroed"])


def test_device_histograms_equal_the_host_form(engine):
    from irec.io import hist_rows
    rng = np.random.default_rng(9)
    # bins in LDS | index values past the LDS bins, count bins past theirs (both go to global memory at once) | one row
    for n, bpr, mk, niv, ncv, hi in ((300, (4, 1, 7), 9, 20, 8, 25), (70, (2,) * 64, 5, 10000, 70, 10050), (1, (1,), 3, 5, 4, 5)):
        T = sum(bpr)
        K = rng.integers(-1, mk + 3, (n, T)).astype(np.int32)
        idx = rng.integers(-2, hi, (n, T, mk)).astype(np.int32)
        host = hist_rows(K, idx, bpr, niv, ncv)
        both = _dev(C.joined(K, idx)).view(n, T, 1 + mk)
        dev = hist_rows(_dev(K), _dev(idx), bpr, niv, ncv)
        dev = hist_rows(both[..., 0], both[..., 1:], bpr, niv, ncv, into=dev)          # accumulated, from the joined-tensor strides
        host = hist_rows(K, idx, bpr, niv, ncv, into=host)
        got = dev.numpy()
        assert host.rejected[0] > 0 or n == 1
        for x, y in zip((got.index, got.counts, got.streams, got.rejected), (host.index, host.counts, host.streams, host.rejected)):
            assert np.array_equal(x, y)


# ---- the models: fit -> compress_rec(tables=) -> decompress, against the round trip without tables ----------------------------------------
SEED = 42


@functools.lru_cache(maxsize=None)
def _rvae():
    from irec.models import BidirectionalResNetVAE
    torch.manual_seed(0)
    m = BidirectionalResNetVAE(num_res_blocks=2, sampler="beam_search", sampler_args={"n_beams": 20, "extra_samples": 1.2},
                               coder_args={"block_size": 1000}, deterministic_filters=8, stochastic_filters=4, kl_per_partition=3.)
    with torch.no_grad():
        m._generative_base.normal_(0, 0.5)
    m = m.cuda().eval()
    torch.manual_seed(7)
    return m, torch.rand(3, 3, 32, 32, device="cuda") - 0.5


def test_rvae_fit_compress_decompress(engine):
    from irec import harness
    from irec.coding import CodingError
    m, images = _rvae()
    tables = harness.fit_symbol_tables(m, images, SEED)
    assert tables.n_res_blocks == 2 and tables.index_counts is not None and int(tables.index_counts.sum()) > tables.index_counts.size
    blob0, off0, recon0 = m.compress_rec(images, SEED)
    blob, off, recon = m.compress_rec(images, SEED, tables=tables)
    assert torch.equal(recon, recon0)
    head = blob.cpu().numpy()[:28]
    assert head[22:26].tolist() == [1, 0, 1, 0]
    print("rvae bytes per image, default:", np.diff(off0.cpu().numpy()).tolist(), "fitted:", np.diff(off.cpu().numpy()).tolist())
    plain = m.decompress_rec(blob0, off0, SEED, tuple(images.shape))
    back = m.decompress_rec_tables(blob, off, SEED, tuple(images.shape), tables)
    assert torch.equal(back, plain)
    both = m.decompress_rec_tables(torch.cat([blob, blob0]), torch.cat([off, off0[1:] + off[-1]]), SEED, (6, 3, 32, 32), tables)
    assert torch.equal(both[:3], both[3:])                                # flagged and unflagged files in one call (one batch of six)
    _, status = m.decompress_rec(blob, off, SEED, tuple(images.shape), strict=False)
    assert status.tolist() == [5, 5, 5]
    with pytest.raises(CodingError, match=r"empirical count tables.*\(image 0\)"):
        m.decompress_rec(blob, off, SEED, tuple(images.shape))


def test_rvae_harness_round_trip_through_files(engine, tmp_path):
    from irec import harness
    m, images = _rvae()
    tables = harness.fit_symbol_tables(m, images, SEED, batch=2)
    one = harness.fit_symbol_tables(m, images, SEED)
    assert np.array_equal(tables.index_counts, one.index_counts) and all(np.array_equal(a, b) for a, b in zip(tables.num_aux_var_counts, one.num_aux_var_counts))
    names_h, names_d = [f"h{i}" for i in range(3)], [f"d{i}" for i in range(3)]
    rows_h = harness.compress_images(m, images, names_h, SEED, 1000, str(tmp_path), tables=tables)
    rows_d = harness.compress_images(m, images, names_d, SEED, 1000, str(tmp_path), rec_on_device=True, tables=tables)
    assert all(r["indices_recovered"] for r in rows_h + rows_d)
    for a, b in zip(names_h, names_d):
        assert (tmp_path / f"{a}.rec").read_bytes() == (tmp_path / f"{b}.rec").read_bytes()
    rows_0 = harness.compress_images(m, images, [f"p{i}" for i in range(3)], SEED, 1000, str(tmp_path), rec_on_device=True)
    plain, _ = harness.decompress_images(m, [str(tmp_path / f"p{i}.rec") for i in range(3)])
    back, rows = harness.decompress_images_tables(m, [str(tmp_path / f"{a}.rec") for a in names_h], tables)
    assert torch.equal(back, plain) and all(r["status"] == 0 for r in rows)
    _, rows = harness.decompress_images(m, [str(tmp_path / f"{a}.rec") for a in names_h], strict=False)
    assert [r["status"] for r in rows] == [5, 5, 5]
    assert len(rows_0) == 3


@functools.lru_cache(maxsize=None)
def _lossy():
    import irec
    from irec.models import Large2LevelVAE
    torch.manual_seed(3)
    m = Large2LevelVAE(level_1_filters=8, level_2_filters=4).cuda().eval()
    with torch.no_grad():                         # the heads of the two posteriors' locs: a larger scale, a larger KL at that level
        for mod in (m.hyper_analysis_transform[-1], m._level_1_posterior_loc_combiner):
            mod.weight.mul_(16.)
            mod.bias.mul_(16.)
    torch.manual_seed(11)
    return m, irec.BeamSearchCoder(kl_per_partition=3., n_beams=10, extra_samples=1., block_size=5), (torch.rand(3, 3, 64, 64) - 0.5).cuda()


@pytest.mark.parametrize("on_device", [False, True], ids=["host_leg", "device_leg"])
def test_lossy_fit_compress_decompress_and_harness(engine, on_device, tmp_path):
    from irec import harness
    m, sampler, images = _lossy()
    tables = harness.fit_symbol_tables_lossy(m, sampler, images, SEED, 5)
    assert tables.n_res_blocks == 2
    blob0, off0, recon0 = m.compress_rec(images, SEED, sampler, rec_on_device=on_device)
    blob, off, recon = m.compress_rec(images, SEED, sampler, rec_on_device=on_device, tables=tables)
    sizes = lambda o: np.diff(o.cpu().numpy() if hasattr(o, "cpu") else o).tolist()
    print("lossy bytes per image, default:", sizes(off0), "fitted:", sizes(off))
    assert torch.equal(recon, recon0)
    shape = tuple(images.shape)
    plain = m.decompress_rec(blob0, off0, SEED, shape, sampler, rec_on_device=on_device)
    back = m.decompress_rec(blob, off, SEED, shape, sampler, rec_on_device=on_device, tables=tables)
    assert torch.equal(back, plain)
    _, status = m.decompress_rec(blob, off, SEED, shape, sampler, rec_on_device=on_device, strict=False)
    assert status.tolist() == [5, 5, 5]
    names = [f"l{i}" for i in range(3)]
    rows = harness.compress_images_lossy(m, sampler, images, names, SEED, 5, str(tmp_path), rec_on_device=on_device, tables=tables)
    assert all(r["indices_recovered"] for r in rows)
    paths = [str(tmp_path / f"{nm}.rec") for nm in names]
    got, rows = harness.decompress_images_lossy(m, sampler, paths, rec_on_device=on_device, tables=tables)
    assert torch.equal(got, plain) and all(r["status"] == 0 for r in rows)
    _, rows = harness.decompress_images_lossy(m, sampler, paths, rec_on_device=on_device, strict=False)
    assert [r["status"] for r in rows] == [5, 5, 5]
