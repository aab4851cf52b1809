"""DLWP (cubed-sphere U-Net) on gfx950 kernels: spec, engine, checkpoint converter, TimeLoop."""
