"""FengWu (cross-modal Swin transformer) on gfx950 kernels: spec, engine, checkpoint reader, TimeLoop."""
