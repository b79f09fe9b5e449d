from smirk_amd.mica import MICA, MappingNetwork  # noqa: F401
