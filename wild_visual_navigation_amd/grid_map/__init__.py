from .grid_map import CarrotGoal, SmartCarrot, TraversabilityGridMap, layer_from_message, layer_to_message  # noqa: F401
