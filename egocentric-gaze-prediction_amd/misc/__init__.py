"""Mirrors of the reference's misc/ scripts (GTEA Gaze dataset preparation)."""
