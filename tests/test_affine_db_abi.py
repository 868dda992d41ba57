"""The A/B switch of the affine database-search kernel (sw_affine_prof_kernel) is an option of the library: listed by
mi355_sw_option_names, so that mi355_sw_set_option and the environment take it.  No GPU."""


def test_no_affine_prof_is_an_option(pgs):
    names = pgs.capi.option_names()
    assert "no_affine_prof" in names and "no_affine_sweep" in names
    assert len(names) == len(set(names))
