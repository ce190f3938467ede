"""``Payne.testing``: checks of a trained network file (testspec.TestSpec)."""
