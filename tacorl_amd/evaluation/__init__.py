"""Rollout-time drivers of the trained modules (reference evaluation/)."""
