"""Training-time utilities under the reference's module paths (reference utils/)."""
