from dvmvs.baselines.runner import main

if __name__ == "__main__":
    main("dpsnet")
