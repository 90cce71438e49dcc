"""Alias of sketch2img_amd.anime2sketch (the reference imports `anime2sketch.model`)."""
from sketch2img_amd.anime2sketch import UnetGenerator, create_model, generate_sketch, sketch_latents  # noqa: F401
