"""FourCastNet v1 (AFNO) on the gfx950 kernels of include/skyrim_fcn.h."""
