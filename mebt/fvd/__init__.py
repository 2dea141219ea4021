"""import-name alias: `mebt.fvd` (reference mebt/fvd/) -> the MI355X-native FVD / KVD evaluation in mebt_amd"""
