"""The thin lens's host side, runnable without a GPU: rtw_lens_rays against the NumPy model of the ray (tests/lens_support.py), the
rejection sampling of the lens point, the optics of the ray, the validation rules and the set / get round trips."""
import numpy as np
import pytest

import raytracerwin_amd as R
import camera_support as CS
import lens_support as LS

f32 = np.float32
W, H, SEED = 96, 54, 12345
PIX = np.arange(W * H)


def lens_of(pose, radius=0.2):
    return R.Lens(radius, LS.target_distance(CS.POSES[pose]))


def lens2(lens):
    return (lens.aperture_radius, lens.focus_distance)


@pytest.mark.parametrize("pose", ["offaxis", "inside"])
def test_lens_rays_match_the_model_exactly(pose):
    cam, lens = CS.camera_of(R, pose), lens_of(pose)
    for p in (0, 3):
        for sub in range(4):
            got = R.lens_rays(cam, lens, W, H, PIX, p, sub, SEED)
            want = LS.model_rays(cam.as_array(), lens2(lens), W, H, PIX, p, sub, SEED)
            assert (LS.bits(got) == LS.bits(want)).all(), (p, sub)


@pytest.mark.parametrize("pose", ["default", "offaxis", "inside"])
def test_radius_zero_is_camera_rays_bit_for_bit(pose):
    cam = CS.camera_of(R, pose)
    for p, sub in ((0, 0), (3, 2)):
        want = R.camera_rays(cam, W, H, PIX, p, sub, SEED)
        assert (LS.bits(R.lens_rays(cam, R.Lens(0.0, 3.0), W, H, PIX, p, sub, SEED)) == LS.bits(want)).all()
        assert (LS.bits(R.lens_rays(cam, None, W, H, PIX, p, sub, SEED)) == LS.bits(want)).all()


def test_samples_that_reject_their_first_try_are_there_and_match_the_model():
    """about 21 % of the samples (1 - pi / 4) need a second try: the library's origins are the model's for exactly those too, and a
    sample that needed another try does not sit where its first try would have put it"""
    cam, lens = CS.camera_of(R, "offaxis"), lens_of("offaxis")
    c = cam.as_array()
    lx, ly, tries = LS.lens_points(PIX, 1, 2, SEED)
    later = tries > 0
    assert 0.15 * len(PIX) < later.sum() < 0.28 * len(PIX) and (tries < LS.TRIES).all()
    got = R.lens_rays(cam, lens, W, H, PIX, 1, 2, SEED)
    # the lens point read back from the library's origins: (origin - eye) . right / radius, to rounding
    off = got[:, 0:3].astype(np.float64) - c[0:3]
    bx, by = off @ c[3:6].astype(np.float64) / lens.aperture_radius, off @ c[6:9].astype(np.float64) / lens.aperture_radius
    assert np.abs(bx - lx).max() < 1e-4 and np.abs(by - ly).max() < 1e-4
    assert (bx * bx + by * by <= 1.0 + 1e-4).all()
    want = LS.model_rays(c, lens2(lens), W, H, PIX, 1, 2, SEED)
    assert (LS.bits(got[later]) == LS.bits(want[later])).all()


def test_eight_rejections_fall_back_to_the_centre():
    out = f32(0.9)                                                  # 0.9^2 + 0.9^2 > 1: outside the disc
    lx = np.full((LS.TRIES, 4), out, f32)
    ly = np.full((LS.TRIES, 4), out, f32)
    lx[0, 0], ly[0, 0] = 0.5, 0.5                                   # sample 0: the first try
    lx[7, 1], ly[7, 1] = -0.25, 0.125                               # sample 1: the last try
    lx[3, 2], ly[3, 2] = 1.0, 0.0                                   # sample 2: exactly on the rim (<= 1) at try 3, and inside again later
    lx[5, 2], ly[5, 2] = 0.1, 0.1
    x, y, t = LS.pick_lens_point(lx, ly)                            # sample 3: never
    assert list(t) == [0, 7, 3, LS.TRIES]
    assert list(x) == [f32(0.5), f32(-0.25), f32(1.0), f32(0.0)] and list(y) == [f32(0.5), f32(0.125), f32(0.0), f32(0.0)]


def test_rays_of_one_pixel_meet_in_the_focal_plane():
    """optics: the point at depth focus_distance along `forward` on each of a pixel's 64 samples' rays is eye + v * s, the point the
    pinhole ray of the same jitter meets that plane in.  Coordinates are below 16 and each point takes about ten float32 operations
    (a few 1e-5): 1e-4 absolute."""
    for pose in ("offaxis", "wide"):
        cam, lens = CS.camera_of(R, pose), lens_of(pose, 0.3)
        c = cam.as_array().astype(np.float64)
        eye, fwd, focal = c[0:3], c[9:12], c[12]
        pixel = np.array([17 * W + 23])
        worst, origins = 0.0, []
        for p in range(16):
            for sub in range(4):
                ray = R.lens_rays(cam, lens, W, H, pixel, p, sub, SEED)[0].astype(np.float64)
                v = np.array([a[0] for a in LS.view_vectors(cam.as_array(), W, H, pixel, p, sub, SEED)], np.float64)
                o, d = ray[0:3], ray[3:6]
                t = (lens.focus_distance - (o - eye) @ fwd) / (d @ fwd)
                worst = max(worst, np.abs(o + t * d - (eye + v * (lens.focus_distance / focal))).max())
                assert abs(np.linalg.norm(d) - 1.0) < 1e-6 and ray[6] == 1000.0
                origins.append(o)
        assert worst < 1e-4, worst
        # origins lie within aperture_radius of the eye, in the plane spanned by right and up -- and they spread over the disc
        off = np.array(origins) - eye
        assert (np.linalg.norm(off, axis=1) <= lens.aperture_radius * (1 + 1e-5)).all()
        assert np.abs(off @ fwd).max() < 1e-5
        assert np.linalg.norm(off, axis=1).max() > 0.5 * lens.aperture_radius and len(np.unique(off.round(6), axis=0)) == 64


def test_every_validation_rule_returns_its_error():
    def bad(fn, *args):
        with pytest.raises(R.RtwError) as e:
            fn(*args)
        assert e.value.code == -1
    s = R.RayTracerScene(None)
    cam = CS.camera_of(R, "offaxis")
    for lens in (R.Lens(-0.1, 2.0), R.Lens(0.1, 0.0), R.Lens(0.1, -3.0), R.Lens(float("nan"), 2.0), R.Lens(0.1, float("inf")),
                 R.Lens(float("inf"), 2.0), R.Lens(0.0, 0.0), R.Lens(0.0, float("nan"))):
        bad(s.set_lens, lens)
        bad(R.lens_rays, cam, lens, W, H, PIX[:4])
    assert s.get_lens() == R.Lens(0.0, 1.0)                         # a refused lens changes nothing
    with pytest.raises(R.RtwError) as e:                            # bit 31 of the sample word belongs to the lens stream
        R.lens_rays(cam, R.Lens(0.1, 2.0), W, H, PIX[:4], 1 << 29)
    assert e.value.code == -6
    R.lens_rays(cam, R.Lens(0.0, 2.0), W, H, PIX[:4], 1 << 29)      # ... the pinhole has no such limit
    s.close()


def test_set_get_round_trips_and_none_restores_the_pinhole():
    s = R.RayTracerScene(None)
    assert s.get_lens() == R.Lens(0.0, 1.0) and s.get_lens().aperture_radius == 0.0
    lens = R.Lens(0.15, 6.5)
    s.set_lens(lens)
    assert s.get_lens() == lens and lens2(s.get_lens()) == (f32(0.15), f32(6.5))
    s.set_lens(R.Lens(0.0, 4.0))                                    # aperture 0: the pinhole, the struct is kept as given
    assert s.get_lens() == R.Lens(0.0, 4.0)
    s.set_lens(lens)
    s.set_lens(None)
    assert s.get_lens() == R.Lens(0.0, 1.0)
    s.set_camera(CS.camera_of(R, "below"))                          # camera and lens are independent settings
    s.set_lens(lens)
    assert s.get_camera() == CS.camera_of(R, "below") and s.get_lens() == lens
    s.close()
