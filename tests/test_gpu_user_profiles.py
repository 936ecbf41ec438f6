"""GPU: native.user_profiles (ncf_user_profiles, csrc/user_profiles.hip) against the float64 contract of tests/user_profiles_ref.py
rounded to fp32 — torch.equal, on both access forms (16-byte loads: F, ld multiples of 4 and aligned bases; single floats: the rest),
every row length around the 8 rows a wave keeps in flight, one user and many, a second call, and the out-of-range column."""
import functools

import numpy as np
import pytest
import torch

from user_profiles_ref import F_LIST, N_ITEMS, N_USERS, cases, make_case, profiles_loop, user_lengths

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _cases(F):
    """(name, case, reference) of one width: computed once, shared by the tests, never written."""
    return [(name, c, profiles_loop(**c)) for name, c in cases(F)]


def _run(gpu, c, pad, shift=0):
    """The kernel over ``c`` with feature and output rows of F + pad floats starting ``shift`` floats into their buffers; returns the
    (U, F) result on the host after checking that nothing else of the output buffer was written."""
    from deeprecommendation_amd import native
    I, F = c["features"].shape
    U = len(c["avg"])
    wide = torch.full((I, F + pad), 7.5)
    wide[:, shift:shift + F] = torch.from_numpy(c["features"])
    feat = wide.to(gpu)[:, shift:shift + F]
    buf = torch.full((U, F + pad), -123.0, device=gpu)
    out = native.user_profiles(*(torch.from_numpy(c[k]).to(gpu) for k in ("rowptr", "col", "rating", "avg")), feat, out=buf[:, shift:shift + F])
    assert out.data_ptr() == buf[:, shift:shift + F].data_ptr() and out.stride(0) == F + pad
    host = buf.cpu()
    assert (host[:, :shift] == -123.0).all() and (host[:, shift + F:] == -123.0).all()
    return host[:, shift:shift + F].contiguous()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("F", F_LIST)
def test_profiles_are_the_float64_contract_bit_for_bit(gpu, F):
    from deeprecommendation_amd import native
    for name, c, ref in _cases(F):
        for pad in (0, 5):
            got = _run(gpu, c, pad)
            assert _same_bits(got, torch.from_numpy(ref)), (name, pad)
            assert _same_bits(_run(gpu, c, pad), got), (name, pad)              # a second call: identical bits
    native.check_oob(gpu)                                                        # no column was out of range


def test_wrapper_allocates_and_handles_an_empty_user_list(gpu):
    from deeprecommendation_amd import native
    name, c, ref = _cases(67)[0]
    dev = {k: torch.from_numpy(v).to(gpu) for k, v in c.items()}
    out = native.user_profiles(dev["rowptr"], dev["col"], dev["rating"], dev["avg"], dev["features"])
    assert out.shape == (N_USERS, 67) and out.is_contiguous() and _same_bits(out.cpu(), torch.from_numpy(ref))
    none = native.user_profiles(dev["rowptr"][:1], dev["col"][:0], dev["rating"][:0], dev["avg"][:0], dev["features"])
    assert none.shape == (0, 67)


@pytest.mark.parametrize("F,pad,shift", [(64, 8, 0), (64, 8, 1), (260, 4, 0), (256, 4, 2)])
def test_aligned_and_misaligned_views_of_wider_buffers(gpu, F, pad, shift):
    """ld a multiple of 4 that is not F: 16-byte accesses at shift 0, single floats when the view starts off a 16-byte boundary."""
    name, c, ref = _cases(F)[0]
    assert _same_bits(_run(gpu, c, pad, shift), torch.from_numpy(ref))


@pytest.mark.parametrize("F", [64, 67])
def test_column_out_of_range_sets_the_flag_and_adds_nothing(gpu, F):
    from deeprecommendation_amd import native
    native.check_oob(gpu)
    c = {k: v.copy() for k, v in make_case(F, user_lengths(seed=4), seed=77 + F).items()}
    u = int(np.nonzero(np.diff(c["rowptr"]) == 9)[0][0])
    c["col"][c["rowptr"][u + 1] - 1] = N_ITEMS                                   # the row's last column: one past the catalogue
    ref = profiles_loop(**c)
    clean = profiles_loop(**dict(c, col=np.where(c["col"] == N_ITEMS, 0, c["col"]).astype(np.int32)))
    assert not np.array_equal(ref[u], clean[u]) and np.array_equal(np.delete(ref, u, 0), np.delete(clean, u, 0))
    got = _run(gpu, c, 0)
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    assert _same_bits(got, torch.from_numpy(ref))
    native.check_oob(gpu)                                                        # the flag was cleared by the raise
