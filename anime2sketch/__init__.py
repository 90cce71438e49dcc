"""Alias package: `anime2sketch.model` resolves to sketch2img_amd.anime2sketch (the reference's trainer.py:15 imports
`anime2sketch.model.create_model`)."""
