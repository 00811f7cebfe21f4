"""The two environment variables of the package (csrc/route.h): SEERHIP_ROUTE="key=value,..." forces a route a run would otherwise choose
from its data (a test hook; the library refuses unknown keys), SEERHIP_DEBUG="item,item" turns diagnostics on stderr on."""
import os


def route(key, default=None):
    for item in os.environ.get("SEERHIP_ROUTE", "").split(","):
        k, eq, v = item.partition("=")
        if eq and k == key:
            return v
    return default


def debug(item):
    return item in os.environ.get("SEERHIP_DEBUG", "").split(",")


def device_list(gpus):
    """The value of --gpus as the devices it names: "a,b,..." as listed (one may be listed twice), a count N as 0 .. N-1; None as None."""
    if gpus is None:
        return None
    return [int(x) for x in gpus.split(",")] if "," in gpus else list(range(int(gpus)))


def device_count(gpus):
    """How many devices --gpus names; a list with an unreadable entry is counted by its entries (the run stops at that entry where the contexts are made)."""
    try:
        return len(device_list(gpus) or ())
    except ValueError:
        if "," not in gpus:
            raise
        return len(gpus.split(","))


def with_route(env_value, **kv):
    """env_value (the current SEERHIP_ROUTE string or None) with the given keys set (value None: removed) -> the new string."""
    items = [it for it in (env_value or "").split(",") if it and it.partition("=")[0] not in kv]
    items += ["%s=%s" % (k, v) for k, v in kv.items() if v is not None]
    return ",".join(items)
