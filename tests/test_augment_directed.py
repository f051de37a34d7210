"""GPU: aug_image_kernel and the grey-mean kernels (csrc/augment.hip) on the directed cases of tests/augment_cases.py -- a colour
lattice through every kind of jitter chain, degenerate resize geometry, grey means of sources large enough for the reduction loop to
go round, mixed batches -- against the float64 restatement, with no seam allowance: a pixel whose hue lies at the 0/360 seam must
match one of its two stated branches.  tests/test_augment_directed_cpu.py shows that a float32 composition meets the same checks
and that each plausible bug fails them.  Run with -s for the worst errors."""
import numpy as np
import pytest
import torch

import augment_cases as K
from orienmask_amd import transform

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _launch(cases, dev, transport_uint8=True):
    """One launch set for `cases`: (images [B,3,H,W] float32, [masks [n,H,W] bool per case]) on the host."""
    res = transform.to_device(transform.collate([K.planned(c, transport_uint8) for c in cases]), dev)
    image, mask = res[0].cpu().numpy(), res[1][3].cpu().numpy()
    first = np.cumsum([0] + [len(c.masks) for c in cases])
    return image, [mask[first[k]:first[k + 1]] for k in range(len(cases))]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def lattice(dev):
    """{source: (cases, images)}: every chain on one source in one launch."""
    return {name: (cases, _launch(cases, dev)[0]) for name, cases in K.lattice_cases().items()}


@pytest.mark.parametrize("name", ["u8", "frac", "wide"])
def test_lattice_every_chain_within_bound_of_a_stated_branch(lattice, name):
    """1331 colours (greys, two-channel ties, both ends of the range) through each op alone, every 2- and 3-op subset and all 24
    orders under three factor sets; uint8 and fractional float32 sources ('wide' leaves [0, 255]: hue does not clip).  Chains
    without hue within 1e-4 of float64, chains with hue within PIXEL_BOUND; a seam pixel within the bound of a or of alt."""
    cases, images = lattice[name]
    no_hue, hue = K.Worst("lattice %s, without hue" % name), K.Worst("lattice %s, with hue" % name)
    for c, got in zip(cases, images):
        (hue if K.bound_of(c) == K.BOUND_HUE else no_hue).add(K.check_image(got, c), c.id)
    print()
    print(no_hue)
    print(hue)


def test_lattice_uint8_hue_first_never_crosses_the_seam(lattice):
    """On integers g - b is exact, so with hue as the first op the device's hue cannot be on the other side of the seam."""
    cases, images = lattice["u8"]
    first = [(c, got) for c, got in zip(cases, images) if c.ops[0][0] == K.H]
    assert len(first) >= 5 + 18
    flagged = 0
    for c, got in first:
        stats = K.check_image(got, c)
        assert stats["alt"] == 0, "%s: %d seam pixels on the other branch" % (c.id, stats["alt"])
        flagged += stats["seam"]
    assert flagged > 0


def test_noop_chain_at_identity_is_the_source_bit_for_bit(dev):
    for c in K.noop_cases():
        got = _launch([c], dev)[0][0]
        assert np.array_equal(_bits(got[:, 0].T), _bits(c.image[0].astype(np.float32))), c.id


def test_geometry_images_pads_and_masks(dev):
    """Each degenerate geometry alone: image within 1e-4 of render_image (saturation then brightness on every tap, no hue), pad
    pixels exactly (float32(pad) - mean) / std, both masks bit-exact to render_masks."""
    worst = K.Worst("geometry")
    for c in K.geometry_cases():
        image, masks = _launch([c], dev)
        worst.add(K.check_image(image[0], c), c.id)
        K.check_pad(image[0], c)
        K.check_masks(masks[0], c)
    print()
    print(worst)


def test_gray_mean_large_sparse_and_tiny_sources(dev):
    """Contrast at f = 0.5 (x / 2 + mean / 2) within 1e-4 of float64 for a 300x500 source (three passes of the reduction loop), 1x257
    (mostly empty workgroups), 1x1 and 16x16, and the 300x500 source with hue and saturation inside the reduction; each image of
    the batch bit-identical to its own launch."""
    cases = K.graymean_cases()
    batch = _launch(cases, dev)[0]
    worst = K.Worst("grey mean")
    for k, c in enumerate(cases):
        worst.add(K.check_image(batch[k], c), c.id)
        K.check_pad(batch[k], c)
        solo = _launch([c], dev)[0][0]
        assert np.array_equal(_bits(batch[k]), _bits(solo)), c.id
    print()
    print(worst)


def test_mixed_batch_bounds_and_bit_identity(dev):
    """Full chain, ops without contrast, no ops, contrast alone and a fractional float32 source in one launch (float32 transport):
    every image within its bound and bit-identical to its own launch; the uint8 subset bit-identical to itself sent as float32."""
    cases = K.batch_cases()
    planned = transform.collate([K.planned(c) for c in cases])
    assert planned.image.dtype == torch.float32 and planned.any_contrast
    batch = _launch(cases, dev)[0]
    worst = K.Worst("mixed batch")
    for k, c in enumerate(cases):
        worst.add(K.check_image(batch[k], c), c.id)
        assert np.array_equal(_bits(batch[k]), _bits(_launch([c], dev)[0][0])), c.id
    assert np.array_equal(_bits(batch[2][:, 0].T), _bits(cases[2].image[0].astype(np.float32)))       # the no-op image, untouched
    sub = cases[:4]
    assert transform.collate([K.planned(c) for c in sub]).image.dtype == torch.uint8
    assert transform.collate([K.planned(c, False) for c in sub]).image.dtype == torch.float32
    u8, f32 = _launch(sub, dev)[0], _launch(sub, dev, transport_uint8=False)[0]
    assert np.array_equal(_bits(u8), _bits(f32)) and np.array_equal(_bits(u8), _bits(batch[:4]))
    print()
    print(worst)
