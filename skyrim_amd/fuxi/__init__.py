"""FuXi (Swin V2 U-Transformer cascade) on gfx950 kernels: spec, engine, checkpoint reader, TimeLoop."""
