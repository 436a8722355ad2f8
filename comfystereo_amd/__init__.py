"""comfystereo_amd -- MI355X-native depth-to-stereo engine, drop-in for ComfyStereo's Stereo Image Node.

Import is cheap and GPU-free; the HIP library is loaded on first use (see _native.lib()).
"""
__version__ = "0.1.0"


def __getattr__(name):
    """NODE_CLASS_MAPPINGS / NODE_DISPLAY_NAME_MAPPINGS, what ComfyUI reads from a custom-node package: the Stereo Image Node's
    and StereoDiffusion's, merged.  Lazy: the node modules (and torch) load when ComfyUI asks, not when the package is imported."""
    if name in ("NODE_CLASS_MAPPINGS", "NODE_DISPLAY_NAME_MAPPINGS"):
        from . import GenerateStereo, stereodiffusion_nodes
        return {**getattr(GenerateStereo, name), **getattr(stereodiffusion_nodes, name)}
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
