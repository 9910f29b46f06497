"""The registry of the device-world families: every world module's ``FAMILY`` record (``worlds.WorldFamily``) by name, in the
order the messages list them, and the lists of names that follow from the records.  A new world is added HERE and nowhere
else outside its own module."""
from . import breakout, cartpole, pendulum, point, pong, snake

FAMILIES = {mod.FAMILY.name: mod.FAMILY for mod in (snake, pong, breakout, point, cartpole, pendulum)}
DEVICE_TYPES = tuple(n + "-device" for n in FAMILIES)
# the lane worlds: their step reports the state an episode ended in (hyps bootstrap_truncated)
LANE_WORLDS = tuple(n for n, f in FAMILIES.items() if f.reports_trunc)
LANE_DEVICE_TYPES = tuple(n + "-device" for n in LANE_WORLDS)
# the families with (1, L) observations: what running normalisation (hyps norm_obs / norm_rewards, section 6m) covers
VECTOR_WORLDS = tuple(n for n, f in FAMILIES.items() if f.vector)
VECTOR_DEVICE_TYPES = tuple(n + "-device" for n in VECTOR_WORLDS)


def family_of(env_type):
    """the record of "Pong-device" / "Pong-host"; None for every other env_type"""
    name, _, where = str(env_type).partition("-")
    return FAMILIES.get(name) if where in ("device", "host") else None
